// resid_carry.h — the tracker's residual memory, DResidualNew: the "last valid fi" propagation of TryVelRot / TryVel.
//
// The reference writes DResidualNew[ikl] = fi for every KeyLine it evaluates, and `fi` is one scalar across the whole loop that only
// a successful match refreshes (global_tracker.cpp:344, 391, 406; TryVel: Residuals[ikl] = fabs(fi)): an evaluated but unmatched
// KeyLine inherits the residual of the last matched KeyLine before it, 0 at the top of the list.  On the device a thread owns one
// KeyLine and the rule is restated by KeyLine status:
//
//   status                       residual buffer entry
//   0  skipped by the gates      0.0 (TryVel: the entry it had) — the reference leaves the entry alone and nothing ever reads it; it
//                                is written anyway so that the wave stores whole lines (with ~13 % of the lanes masked most lines
//                                would be written in part, which the memory system turns into read-modify-write)
//   1  out of image              max_r (TryVelRot only; TryVel has no such entry: status 0)
//   2  evaluated, matched        its own fi — the only VALID value, the one later KeyLines inherit
//   3  evaluated, unmatched      the fi of the last status-2 KeyLine before it, found in three steps:
//        inside its wave           ballot of the valid lanes, the highest one below this lane, one shuffle    wave_last_valid
//        inside its block          the last valid value of the nearest earlier wave that has one, through two
//                                  small LDS arrays (s_whas / s_wlast), one barrier after every wave has
//                                  published                                                                   carry_publish, carry_inherit
//        across blocks             no block waits for another: the entry gets the MARKER, a quiet NaN no
//                                  arithmetic produces (resid_carry_bits, ctx.h), and every reader replaces it by
//                                  the block's carry-in
//
// Every block also stores its last valid value, or the marker if it has none, in block_last[seq][blk] (carry_block_last).  The LM step
// that follows the evaluation (k_lm_step / k_lm_step2 through lm_body, k_lmv_step for TryVel) turns block_last into the row
// resid_carry[buffer][seq][blk] = the last non-marker block_last of the blocks before blk, 0.0 for block 0 and for blocks before the
// first match: up to 64 blocks with wave_last_valid across the lanes, longer lists with a serial loop in one lane.  A block's granule
// is kTvrBlock KeyLines whatever the launch shape.
//
// Who reads a marker back, each as `is_carry(v) ? resid_carry[..][blk] : v`:
//   * the next reweighted evaluation, for its Huber weight (is_carry(rprev) -> carry_in_prev in tvr_body / tvr_body_f32 / tvr_rw2_body,
//     the carry row's entry in k_try_vel),
//   * k_tv_resolve, after the last TryVel evaluation of a minimisation (the buffer is updated in place and kept across frames),
//   * k_resolve_resid, when the host downloads a residual buffer.
// The float tracker keeps float values in the same fp64 buffers (exactly representable), widened at the store: marker and carries are shared.
#pragma once
#include "ctx.h"

namespace edgehip {

__device__ __forceinline__ double carry_marker() { return __longlong_as_double((long long)resid_carry_bits()); }
__device__ __forceinline__ bool is_carry(double v) { return __double_as_longlong(v) == (long long)resid_carry_bits(); }

// The wave primitive: among the lanes whose `valid` is set, the highest one below this lane and the highest one of the wave, with
// their values.  (Lane 0's value where there is no such lane: read `inh` behind has_below and `top` behind any.)
// (The value by reference, the flag and the lane by value, the result passed on by value: the compiler simplifies a helper before it
// inlines it, and with this shape the default build's kernels keep the register counts they had with the steps written out.)
template <typename T>
struct WaveLast {
    bool has_below;   // a valid lane lies below this one
    T inh;            // the value of the highest of them
    bool any;         // the wave has a valid lane
    T top;            // the value of the highest valid lane
};
template <typename T>
__device__ __forceinline__ WaveLast<T> wave_last_valid(const T &v, const bool valid, const int lane) {
    WaveLast<T> r;
    const unsigned long long vmask = __ballot(valid);
    const unsigned long long below = vmask & ((1ull << lane) - 1ull);
    const int src = below ? 63 - __clzll(below) : 0;
    r.has_below = below != 0;
    r.inh = __shfl(v, src, 64);
    const int top = vmask ? 63 - __clzll(vmask) : 0;
    r.top = __shfl(v, top, 64);
    r.any = vmask != 0;
    return r;
}

// The block-level steps, over two LDS arrays of the caller ([NW] each, per chain in a two-chain body): every wave publishes, ONE
// barrier of the caller's, then the unmatched KeyLines and the block's last value read.
template <typename T, int NW>
__device__ __forceinline__ void carry_publish(const WaveLast<T> w, const int lane, const int wave, T (&s_wlast)[NW], int (&s_whas)[NW]) {
    if (lane == 0) {
        s_whas[wave] = w.any;
        s_wlast[wave] = w.top;
    }
}
// what an unmatched KeyLine inherits: own wave below, then the earlier waves, else the marker (resolved from the block carries)
template <typename T, int NW>
__device__ __forceinline__ double carry_inherit(const WaveLast<T> w, const int wave, const T (&s_wlast)[NW], const int (&s_whas)[NW]) {
    double v = carry_marker();
    bool have = false;
    if (w.has_below) { v = (double)w.inh; have = true; }
    for (int pw = wave - 1; pw >= 0 && !have; pw--)
        if (s_whas[pw]) { v = (double)s_wlast[pw]; have = true; }
    return v;
}
// last valid value of the whole block (marker if none), for the carries of the following blocks
template <typename T, int NW>
__device__ __forceinline__ double carry_block_last(const T (&s_wlast)[NW], const int (&s_whas)[NW]) {
    double bl = carry_marker();
    for (int pw = NW - 1; pw >= 0; pw--)
        if (s_whas[pw]) { bl = (double)s_wlast[pw]; break; }
    return bl;
}

}  // namespace edgehip
