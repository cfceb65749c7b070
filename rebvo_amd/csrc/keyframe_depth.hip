// keyframe_depth.hip — depth moves along the key-frame links: the reference's kfvo::mapKFUsingIDK / mapKLUsingIDK
// (src/mtracklib/kfvo.cpp:1147-1184, 1276-1360, through rotateQs, include/mtracklib/kfvo.h:68-81), translateDepth_F2KF with
// optimizeScaleBack (:653-686, 305-341), translateDepth_KF2F (:607-634) and translateDepth_New2Old (:637-650), for every sequence's
// current key frame (keyframe_track.hip) against a ring slot, and along the key-frame list (keyframe_list.hip), for whole batches.
// Upstream defines these and never calls them; nothing here runs unless a caller calls it.
//
//   k_kd_rows<MODE>   one thread per walked KeyLine and tile, grid (ceil(max_points / 256 / tiles), nseq) with tiles in [1, 8] by the batch's size
//            (kd_tiles): a block never straddles two sequences, thread 0
//            forms the relative pose once (TooN's products: row dot products, 0 += in index order) and hands the 12 doubles to the block
//            through LDS.  The walked list's link column and the written fields stream coalesced (the key frames and ring slots are
//            SoA); the partner is the one gather.  MODE 0 mapKFUsingIDK, 1 translateDepth_F2KF without the scale step, 2
//            translateDepth_KF2F, 3 one position of translateDepth_New2Old (the walked list and, but for the newest position, the
//            partner are 168-byte records of the list's ring: strided, as the list stores them).
//   k_kd_scale        translateDepth_F2KF with optim_scale: ONE workgroup of 1024 threads per sequence loops over the key frame's rows
//            twice in one launch.  Pass 1: thread t takes rows t, t + 1024, ... in that order and keeps optimizeScaleBack's two sums; the
//            sums go through the wave butterfly (lane ^ 32, 16, 8, 4, 2, 1, the order of wave_reduce.h), then the 16 waves are added in
//            index order through LDS: fixed by the row index alone, no float atomics.  Thread 0 divides and writes kf.K.  Pass 2: the
//            rewrite of MODE 1 with the new K.  The partner is fetched again in pass 2 (keeping it in registers was not tried).
//   translateDepth_New2Old   one k_kd_rows<3> launch per position, ascending, per iteration: position i reads position i + 1 and writes
//            position i, and the launch of i + 1 is behind it in the stream, so every position reads its successor as it was before the
//            iteration, and the next iteration reads this one's results: the reference's sequential walk, without a snapshot.
//
// The rules per KeyLine, fp64 in the reference's order (tests/keyframe_depth_port.py restates them); p_m, u_m are the records' floats
// widened, rho and s_rho their doubles:
//   rotateQs(q, R, zf)     qr = R * (q0 / zf, q1 / zf, 1); |qr2| > 0: (qr0 / qr2 * zf, qr1 / qr2 * zf, q2 / qr2, q3 / qr2), else zeros
//   mapKLUsingIDK          q = rotateQs((p_m, rho, s_rho), FRelRot, zf); v = q3^2; p_p = v + (q2 QRel)^2 + QAbs^2; Y = u . (p_b - q01);
//            H = u_x (T0 zf - T2 p_bx) + u_y (T1 zf - T2 p_by); e = Y - H q2; S = H p_p H + LU^2; K = p_p H (1 / S); q2 += K e;
//            q3 = sqrt((1 - K H) p_p); (rho, s_rho) = rotateQs(q, FRelRot^T, zf)[2, 3]; then the clamp chain, an else-if chain with its
//            holes: rho < RHO_MIN: s_rho += RHO_MIN - rho, rho = RHO_MIN (a NaN s_rho stays); rho > RHO_MAX: rho = RHO_MAX; a NaN or
//            infinity in either: (RhoInit, RHO_MAX); s_rho < 0: (RhoInit, RHO_MAX).
//   translate              q2 = 1 / ((BRelRot * unprojectHomCordVec(p_m, rho))_2 * K + BRelPos_2) of the PARTNER (cam_model.h:146-169);
//            rho = q2 * kf.K; F2KF: s_rho = rho * (s_rho_b / rho_b), m_num++; KF2F: s_rho = rho / rho_b * s_rho_b.
//   optimizeScaleBack      kfvo::unProject / kfvo::project (kfvo.h:42-48: one reciprocal, not the camera's divisions): q2 = 1 / ((BRelRot
//            * x)_2 * K + BRelPos_2); for q2 > 0: v = (s_rho_b q2 / rho_b Kr)^2 + s_rho^2 with Kr = kf.K, rTr0 += q2 q2 / v, rTr += q2 rho
//            / v; Kr = rTr / rTr0 when both are > 0, else 1.
#include "keyframe_track.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace edgehip {

constexpr int kKdThreads = 256;
constexpr int kKdScaleThreads = 1024;
constexpr int kKdScaleWaves = kKdScaleThreads / 64;
constexpr double kKdRhoMax = 20.0, kKdRhoMin = 1e-3, kKdRhoInit = 1.0;   // edge_finder.h:38-40

struct KdArgs {
    const KlSoA *kf_kl, *slot_kl;
    const int32_t *slot_kn;
    KfSeq *ks;               // (the scale step writes pose.K)
    const SeqDev *seqs;
    const double *pose_in;   // [nseq][13]: Pose, Pos, K; null: seq_state's
    edgehip_kf_depth *out;   // [nseq], zeroed
    const uint8_t *mask;     // [nseq] edgehip_keyframe_depth_select's; null: every sequence
    KfListDev list;
    int cap, pos, count_on;  // pos: the walked position of the list pass; count_on: this launch's links are counted
    int tiles;               // tiles of 256 KeyLines a block of k_kd_rows takes (kd_grid)
    double zfm, q_abs, q_rel, loc_unc;
};

// A KeyLine list as the rows read it: the arrays of a key frame or ring slot, or the records of a list entry
struct KdView {
    const KlSoA *soa;        // null: records
    edgehip_keyline *rec;
    int n;
};
__device__ __forceinline__ float2 kd_p_m(const KdView &v, int i) { return v.soa ? v.soa->p_m[i] : make_float2(v.rec[i].p_m[0], v.rec[i].p_m[1]); }
__device__ __forceinline__ float2 kd_u_m(const KdView &v, int i) { return v.soa ? v.soa->u_m[i] : make_float2(v.rec[i].u_m[0], v.rec[i].u_m[1]); }
__device__ __forceinline__ double kd_rho(const KdView &v, int i) { return v.soa ? v.soa->rho[i] : v.rec[i].rho; }
__device__ __forceinline__ double kd_s_rho(const KdView &v, int i) { return v.soa ? v.soa->s_rho[i] : v.rec[i].s_rho; }

struct KdRel { double R[9], T[3], K, kfK; };   // the relative pose, the K argument, the walked key frame's K

// The frame's pose: the caller's, or localPose = Pose * R, localPos = Pos - localPose * V * K and K of seq_state (as k_kc_solve takes them)
__device__ __forceinline__ void kd_frame_pose(const KdArgs &a, int seq, double *Pose, double *Pos, double &K) {
    if (a.pose_in) {
        const double *pi = a.pose_in + (size_t)seq * 13;
#pragma unroll
        for (int i = 0; i < 9; i++) Pose[i] = pi[i];
#pragma unroll
        for (int i = 0; i < 3; i++) Pos[i] = pi[9 + i];
        K = pi[12];
        return;
    }
    const edgehip_seq_state &p = a.seqs[seq].pub;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) Pose[r * 3 + c] = p.Pose[r * 3 + 0] * p.R[0 * 3 + c] + p.Pose[r * 3 + 1] * p.R[1 * 3 + c] + p.Pose[r * 3 + 2] * p.R[2 * 3 + c];
#pragma unroll
    for (int i = 0; i < 3; i++) Pos[i] = p.Pos[i] - (Pose[i * 3] * p.V[0] + Pose[i * 3 + 1] * p.V[1] + Pose[i * 3 + 2] * p.V[2]) * p.K;
    K = p.K;
}
// R = A^T * B, T = A^T * (PB - PA): TooN's products, row dot products from 0 in index order
__device__ __forceinline__ void kd_relative(const double *A, const double *PA, const double *B, const double *PB, KdRel &rel) {
    double d[3];
#pragma unroll
    for (int i = 0; i < 3; i++) d[i] = PB[i] - PA[i];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) s += A[k * 3 + r] * B[k * 3 + c];
            rel.R[r * 3 + c] = s;
        }
        double s = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) s += A[k * 3 + r] * d[k];
        rel.T[r] = s;
    }
}

// kfvo::rotateQs; TR: with R^T
template <bool TR>
__device__ __forceinline__ void kd_rotate_qs(const double *q0, const double *R, double zf, double *q1) {
    const double a[3] = {q0[0] / zf, q0[1] / zf, 1.0};
    double qr[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        double s = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) s += (TR ? R[k * 3 + r] : R[r * 3 + k]) * a[k];
        qr[r] = s;
    }
    q1[0] = q1[1] = q1[2] = q1[3] = 0.0;
    if (fabs(qr[2]) > 0) {
        q1[0] = qr[0] / qr[2] * zf;
        q1[1] = qr[1] / qr[2] * zf;
        q1[2] = q0[2] / qr[2];
        q1[3] = q0[3] / qr[2];
    }
}

// kfvo::mapKLUsingIDK (the live definition, kfvo.cpp:1276-1360)
__device__ __forceinline__ void kd_map_row(const KdRel &rel, const KdArgs &a, float2 pm, double &rho, double &s_rho, float2 pb, float2 ub) {
    const double zf = a.zfm;
    const double q0[4] = {(double)pm.x, (double)pm.y, rho, s_rho};
    double q[4];
    kd_rotate_qs<false>(q0, rel.R, zf, q);
    const double qx = q[0], qy = q[1], q0x = (double)pb.x, q0y = (double)pb.y;
    double v_rho = q[3] * q[3];
    const double u_x = (double)ub.x, u_y = (double)ub.y;
    const double rho_p = q[2];
    const double rq = q[2] * a.q_rel;
    const double p_p = v_rho + rq * rq + a.q_abs * a.q_abs;
    const double Y = u_x * (q0x - qx) + u_y * (q0y - qy);
    const double H = u_x * (rel.T[0] * zf - rel.T[2] * q0x) + u_y * (rel.T[1] * zf - rel.T[2] * q0y);
    const double e = Y - H * rho_p;
    const double S = H * p_p * H + a.loc_unc * a.loc_unc;
    const double K = p_p * H * (1 / S);
    q[2] = rho_p + (K * e);
    v_rho = (1 - K * H) * p_p;
    q[3] = sqrt(v_rho);
    double q_up[4];
    kd_rotate_qs<true>(q, rel.R, zf, q_up);
    double r = q_up[2], s = q_up[3];
    if (r < kKdRhoMin) {
        s += kKdRhoMin - r;
        r = kKdRhoMin;
    } else if (r > kKdRhoMax) {
        r = kKdRhoMax;
    } else if (isnan(r) || isnan(s) || isinf(r) || isinf(s)) {
        r = kKdRhoInit;
        s = kKdRhoMax;
    } else if (s < 0) {
        r = kKdRhoInit;
        s = kKdRhoMax;
    }
    rho = r;
    s_rho = s;
}

// q1[2] of cam.projectHomCordVec(BRelRot * cam.unprojectHomCordVec(p_m.x, p_m.y, rho) * K + BRelPos)
__device__ __forceinline__ double kd_reproject_rho(const KdRel &rel, double zfm, float2 pm, double rho) {
    const double x[3] = {(double)pm.x / rho / zfm, (double)pm.y / rho / zfm, 1.0 / rho};
    double s = 0;
    s += rel.R[6] * x[0]; s += rel.R[7] * x[1]; s += rel.R[8] * x[2];
    return 1 / (s * rel.K + rel.T[2]);
}

// The views of a launch: `own` is walked and written, `oth` is what its links index.  A sequence without a key frame, or one that
// edgehip_keyframe_depth_select left out, walks nothing.
template <int MODE>
__device__ __forceinline__ bool kd_views(const KdArgs &a, int seq, KdView &own, KdView &oth, const edgehip_kf_pose *&own_pose, const edgehip_kf_pose *&oth_pose) {
    const KfSeq &k = a.ks[seq];
    own_pose = oth_pose = nullptr;
    if (k.kf_count <= 0 || (a.mask && !a.mask[seq])) return false;
    const int kf_n = max(0, min(k.kn, a.cap));
    if (MODE == 3) {
        const KfListDev &l = a.list;
        const int first = l.ls[seq].first, held = max(0, min(l.ls[seq].held, l.capacity));
        if (a.pos >= held) return false;   // the newest position has no successor
        const size_t e0 = (size_t)seq * l.capacity + (size_t)((first + a.pos) % l.capacity);
        own.soa = nullptr; own.rec = (edgehip_keyline *)(l.rec + e0 * l.stride); own.n = max(0, min(l.hdr[e0].kn, a.cap));
        own_pose = &l.hdr[e0].pose;
        if (a.pos + 1 < held) {
            const size_t e1 = (size_t)seq * l.capacity + (size_t)((first + a.pos + 1) % l.capacity);
            oth.soa = nullptr; oth.rec = (edgehip_keyline *)(l.rec + e1 * l.stride); oth.n = max(0, min(l.hdr[e1].kn, a.cap));
            oth_pose = &l.hdr[e1].pose;
        } else {
            oth.soa = &a.kf_kl[seq]; oth.rec = nullptr; oth.n = kf_n;
            oth_pose = &k.pose;
        }
        return true;
    }
    const int sl_n = max(0, min(a.slot_kn[seq], a.cap));
    own.rec = oth.rec = nullptr;
    if (MODE == 2) { own.soa = &a.slot_kl[seq]; own.n = sl_n; oth.soa = &a.kf_kl[seq]; oth.n = kf_n; }
    else { own.soa = &a.kf_kl[seq]; own.n = kf_n; oth.soa = &a.slot_kl[seq]; oth.n = sl_n; }
    own_pose = &k.pose;
    return true;
}

// thread 0: the relative pose of the launch into LDS
template <int MODE>
__device__ __forceinline__ void kd_lead(const KdArgs &a, int seq, const edgehip_kf_pose *own_pose, const edgehip_kf_pose *oth_pose, KdRel &rel) {
    if (MODE == 3) {   // translateDepth_F2KF(kf0, kf1.edges(), kf1.Pose, kf1.Pos, kf1.K, false)
        kd_relative(own_pose->Pose, own_pose->Pos, oth_pose->Pose, oth_pose->Pos, rel);
        rel.K = oth_pose->K;
        rel.kfK = own_pose->K;
        return;
    }
    double Pose[9], Pos[3], K;
    kd_frame_pose(a, seq, Pose, Pos, K);
    const edgehip_kf_pose &kf = a.ks[seq].pose;
    if (MODE == 1) kd_relative(kf.Pose, kf.Pos, Pose, Pos, rel);   // BRelRot = kf.Pose^T * Pose, BRelPos = kf.Pose^T * (Pos - kf.Pos)
    else kd_relative(Pose, Pos, kf.Pose, kf.Pos, rel);             // Pose^T * kf.Pose, Pose^T * (kf.Pos - Pos)
    rel.K = K;
    rel.kfK = kf.K;
}

// the link of walked row i: -1 unmatched (a link outside the list it indexes among them, which sets guard bit 2)
template <int MODE>
__device__ __forceinline__ int kd_link(const KdView &own, int nb, int i, bool &oob) {
    const int link = own.soa ? (MODE == 2 ? own.soa->m_id_kf[i] : own.soa->m_id_f[i]) : own.rec[i].m_id_f;
    if (link >= nb) { oob = true; return -1; }
    return link;
}

// translateDepth_F2KF's / _KF2F's rewrite of row i from its partner
template <int MODE>
__device__ __forceinline__ void kd_translate_row(const KdRel &rel, double zfm, const KdView &own, const KdView &oth, int i, int link) {
    const double rho_b = kd_rho(oth, link), s_rho_b = kd_s_rho(oth, link);
    const double rho = kd_reproject_rho(rel, zfm, kd_p_m(oth, link), rho_b) * rel.kfK;
    const double s_rho = MODE == 2 ? rho / rho_b * s_rho_b : rho * (s_rho_b / rho_b);
    if (own.soa) {
        own.soa->rho[i] = rho;
        own.soa->s_rho[i] = s_rho;
        if (MODE != 2) own.soa->m_num[i] += 1;
    } else {
        own.rec[i].rho = rho;
        own.rec[i].s_rho = s_rho;
        own.rec[i].m_num += 1;
    }
}

__device__ __forceinline__ void kd_tally(const KdArgs &a, int seq, bool done, bool oob) {
    const int c = __popcll(__ballot(done));
    const bool any_oob = __ballot(oob) != 0;
    if ((threadIdx.x & 63) == 0) {
        if (c && a.count_on) atomicAdd(&a.out[seq].count, c);
        if (any_oob) atomicOr(&a.out[seq].guard, 4);
    }
}

template <int MODE>
__global__ __launch_bounds__(kKdThreads) void k_kd_rows(KdArgs a) {
    __shared__ KdRel rel;
    const int seq = blockIdx.y, first = blockIdx.x * a.tiles * kKdThreads;
    KdView own, oth;
    const edgehip_kf_pose *own_pose, *oth_pose;
    if (!kd_views<MODE>(a, seq, own, oth, own_pose, oth_pose)) return;
    if ((MODE == 1 || MODE == 2) && blockIdx.x == 0 && threadIdx.x == 0) a.out[seq].K = a.ks[seq].pose.K;
    if (first >= own.n) return;
    if (threadIdx.x == 0) kd_lead<MODE>(a, seq, own_pose, oth_pose, rel);
    __syncthreads();
    for (int t = 0; t < a.tiles; t++) {   // (uniform bounds: every lane reaches the ballots of kd_tally)
        const int i = first + t * kKdThreads + (int)threadIdx.x;
        if (i - (int)threadIdx.x >= own.n) break;
        bool done = false, oob = false;
        if (i < own.n) {
            const int link = kd_link<MODE>(own, oth.n, i, oob);
            if (link >= 0) {
                done = true;
                if (MODE == 0) {
                    double rho = own.soa->rho[i], s_rho = own.soa->s_rho[i];
                    kd_map_row(rel, a, own.soa->p_m[i], rho, s_rho, kd_p_m(oth, link), kd_u_m(oth, link));
                    own.soa->rho[i] = rho;
                    own.soa->s_rho[i] = s_rho;
                } else {
                    kd_translate_row<MODE>(rel, a.zfm, own, oth, i, link);
                }
            }
        }
        kd_tally(a, seq, done, oob);
    }
}

__device__ __forceinline__ double kd_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(kKdScaleThreads) void k_kd_scale(KdArgs a) {
    __shared__ KdRel rel;
    __shared__ double part[kKdScaleWaves][2];
    const int seq = blockIdx.x;
    KdView own, oth;
    const edgehip_kf_pose *own_pose, *oth_pose;
    if (!kd_views<1>(a, seq, own, oth, own_pose, oth_pose)) return;
    if (threadIdx.x == 0) kd_lead<1>(a, seq, own_pose, oth_pose, rel);
    __syncthreads();
    // optimizeScaleBack's sums
    double rTr = 0, rTr0 = 0;
    bool oob = false;
    const double Kr = rel.kfK;
    for (int i = threadIdx.x; i < own.n; i += kKdScaleThreads) {
        const int link = kd_link<1>(own, oth.n, i, oob);
        if (link < 0) continue;
        const float2 pm = oth.soa->p_m[link];
        const double rho = oth.soa->rho[link], s_rho = oth.soa->s_rho[link];
        const double iz = 1 / rho;
        const double x[3] = {(double)pm.x / a.zfm * iz, (double)pm.y / a.zfm * iz, 1.0 * iz};
        double s = 0;
        s += rel.R[6] * x[0]; s += rel.R[7] * x[1]; s += rel.R[8] * x[2];
        const double q2 = 1.0 * (1 / (s * rel.K + rel.T[2]));
        if (q2 > 0) {
            const double w = s_rho * q2 / rho * Kr, s_b = own.soa->s_rho[i];
            const double v = w * w + s_b * s_b;
            rTr0 += q2 * q2 / v;
            rTr += q2 * own.soa->rho[i] / v;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    rTr0 = kd_wave_sum(rTr0);
    rTr = kd_wave_sum(rTr);
    if (lane == 0) { part[wave][0] = rTr0; part[wave][1] = rTr; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s0 = 0, s1 = 0;
        for (int w = 0; w < kKdScaleWaves; w++) { s0 += part[w][0]; s1 += part[w][1]; }
        const double Kn = (s0 > 0 && s1 > 0) ? (s1 / s0) : 1;
        edgehip_kf_depth &o = a.out[seq];
        if (isfinite(Kn)) { a.ks[seq].pose.K = Kn; rel.kfK = Kn; }
        else atomicOr(&o.guard, 1);
        o.K = rel.kfK; o.rTr = s1; o.rTr0 = s0;
    }
    __syncthreads();
    // the rewrite
    int count = 0;
    for (int i = threadIdx.x; i < own.n; i += kKdScaleThreads) {
        bool again = false;
        const int link = kd_link<1>(own, oth.n, i, again);
        if (link < 0) continue;
        kd_translate_row<1>(rel, a.zfm, own, oth, i, link);
        count++;
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) count += __shfl_xor(count, off, 64);
    if (lane == 0 && count) atomicAdd(&a.out[seq].count, count);
    if (__ballot(oob) != 0 && lane == 0) atomicOr(&a.out[seq].guard, 4);
}

}  // namespace edgehip

using namespace edgehip;

// ---- scratch: the caller's poses on their way in and the results on their way out; allocated by the first call, freed with the key frames
void edgehip::kf_depth_free(edgehip_ctx *c) {
    auto *d = c->kftrack;
    if (!d) return;
    if (d->kd_pose_dev) (void)hipFree(d->kd_pose_dev);
    if (d->kd_out_dev) (void)hipFree(d->kd_out_dev);
    if (d->kd_mask_dev) (void)hipFree(d->kd_mask_dev);
    if (d->kd_pose_host) (void)hipHostFree(d->kd_pose_host);
    for (hipEvent_t &e : d->kd_ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
    d->kd_pose_dev = nullptr; d->kd_out_dev = nullptr; d->kd_pose_host = nullptr; d->kd_mask_dev = nullptr;
    d->kd_busy = d->kd_timed = d->kd_masked = false;
}

static int kd_scratch(edgehip_ctx *c, const char *who) {
    auto *d = c->kftrack;
    if (d->kd_out_dev) return 0;
    const size_t B = c->plan.nseq;
    bool ok = hipMalloc((void **)&d->kd_pose_dev, 8 * 13 * B) == hipSuccess && hipMalloc((void **)&d->kd_out_dev, sizeof(edgehip_kf_depth) * B) == hipSuccess &&
              hipMalloc((void **)&d->kd_mask_dev, B) == hipSuccess && hipHostMalloc((void **)&d->kd_pose_host, 8 * 13 * B, hipHostMallocDefault) == hipSuccess;
    for (int j = 0; j < 3 && ok; j++) ok = (j < 2 ? hipEventCreate(&d->kd_ev[j]) : hipEventCreateWithFlags(&d->kd_ev[j], hipEventDisableTiming)) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        kf_depth_free(c);
        set_error(std::string(who) + ": scratch allocation failed (137 B x nseq)");
        return EDGEHIP_ERR_MEMORY;
    }
    return 0;
}

// A block forms the relative pose once (one lane, the others wait), so a large batch gives a block several tiles of 256 KeyLines: as many
// as keep about kKdBlocks blocks in the grid, 8 at the most; a small batch keeps one tile per block and fills the device.
constexpr int kKdBlocks = 8192;
static int kd_tiles(edgehip_ctx *c) {
    const long tiles = ((long)c->plan.cap + kKdThreads - 1) / kKdThreads * c->plan.nseq;
    return (int)std::max(1L, std::min(8L, tiles / kKdBlocks));
}

static KdArgs kd_args(edgehip_ctx *c, int slot) {
    auto *d = c->kftrack;
    KdArgs a;
    a.kf_kl = d->kl_dev; a.slot_kl = kldev(c, slot);
    a.slot_kn = c->kn_slot + (size_t)slot * c->plan.nseq;
    a.ks = d->ks; a.seqs = c->seq;
    a.pose_in = nullptr;
    a.out = d->kd_out_dev;
    a.mask = d->kd_masked ? d->kd_mask_dev : nullptr;
    a.list = d->list;
    a.cap = c->plan.cap; a.pos = 0; a.count_on = 1; a.tiles = kd_tiles(c);
    a.zfm = c->plan.zfm; a.q_abs = a.q_rel = a.loc_unc = 0;
    return a;
}

// Pose[nseq][9] | Pos[nseq][3] | K[nseq] (null: 1) -> the device's [nseq][13] rows, through the page-locked row: the caller's arrays are
// free on return and nothing waits for the stream
static int kd_push_pose(edgehip_ctx *c, const double *Pose, const double *Pos, const double *K, KdArgs &a) {
    auto *d = c->kftrack;
    if (!Pose) return 0;
    const size_t B = c->plan.nseq;
    if (d->kd_busy) EH_CHECK(hipEventSynchronize(d->kd_ev[2]));
    d->kd_busy = false;
    for (size_t s = 0; s < B; s++) {
        memcpy(d->kd_pose_host + s * 13, Pose + s * 9, 72);
        memcpy(d->kd_pose_host + s * 13 + 9, Pos + s * 3, 24);
        d->kd_pose_host[s * 13 + 12] = K ? K[s] : 1.0;
    }
    EH_CHECK(hipMemcpyAsync(d->kd_pose_dev, d->kd_pose_host, 8 * 13 * B, hipMemcpyHostToDevice, c->stream));
    EH_CHECK(hipEventRecord(d->kd_ev[2], c->stream));
    d->kd_busy = true;
    a.pose_in = d->kd_pose_dev;
    return 0;
}

static int kd_begin(edgehip_ctx *c) {
    auto *d = c->kftrack;
    EH_CHECK(hipMemsetAsync(d->kd_out_dev, 0, sizeof(edgehip_kf_depth) * c->plan.nseq, c->stream));
    EH_CHECK(hipEventRecord(d->kd_ev[0], c->stream));
    return 0;
}
// out == NULL: nothing is waited for
static int kd_end(edgehip_ctx *c, edgehip_kf_depth *out) {
    auto *d = c->kftrack;
    EH_CHECK(hipEventRecord(d->kd_ev[1], c->stream));
    d->kd_timed = true;
    if (!out) return 0;
    EH_CHECK(hipMemcpyAsync(out, d->kd_out_dev, sizeof(edgehip_kf_depth) * c->plan.nseq, hipMemcpyDeviceToHost, c->stream));
    EH_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}
static dim3 kd_grid(edgehip_ctx *c) {
    const int tiles = (c->plan.cap + kKdThreads - 1) / kKdThreads, per = kd_tiles(c);
    return dim3((unsigned)((tiles + per - 1) / per), (unsigned)c->plan.nseq);
}

// behind kf_entry: whatever these return, the caller then says it is done with the slot
static int kd_map_run(edgehip_ctx *c, int slot_new, const double *Pose, const double *Pos, double q_abs, double q_rel, double loc_unc, edgehip_kf_depth *out) {
    if (int e = kd_scratch(c, "keyframe_map_depth")) return e;
    KdArgs a = kd_args(c, slot_new);
    a.q_abs = q_abs; a.q_rel = q_rel; a.loc_unc = loc_unc;
    if (int e = kd_push_pose(c, Pose, Pos, nullptr, a)) return e;
    if (int e = kd_begin(c)) return e;
    hipLaunchKernelGGL(k_kd_rows<0>, kd_grid(c), dim3(kKdThreads), 0, c->stream, a);
    EH_LAUNCH_CHECK();
    return kd_end(c, out);
}

static int kd_translate_run(edgehip_ctx *c, int slot_new, int direction, const double *Pose, const double *Pos, const double *K, int optim_scale,
                            edgehip_kf_depth *out) {
    if (int e = kd_scratch(c, "keyframe_translate_depth")) return e;
    KdArgs a = kd_args(c, slot_new);
    if (int e = kd_push_pose(c, Pose, Pos, K, a)) return e;
    if (int e = kd_begin(c)) return e;
    if (direction) hipLaunchKernelGGL(k_kd_rows<2>, kd_grid(c), dim3(kKdThreads), 0, c->stream, a);
    else if (optim_scale) hipLaunchKernelGGL(k_kd_scale, dim3((unsigned)c->plan.nseq), dim3(kKdScaleThreads), 0, c->stream, a);
    else hipLaunchKernelGGL(k_kd_rows<1>, kd_grid(c), dim3(kKdThreads), 0, c->stream, a);
    EH_LAUNCH_CHECK();
    if (direction)   // the slot's rho / s_rho changed: a stage-level call on the stage-A stream sees them
        if (int e = order_a_after_bc(c)) return e;
    return kd_end(c, out);
}

int edgehip_keyframe_map_depth(edgehip_ctx *c, int slot_new, const double *Pose, const double *Pos, double reshape_q_abs, double reshape_q_rel,
                               double location_uncertainty, edgehip_kf_depth *out) {
    EH_ENTER(c);
    if ((Pose != nullptr) != (Pos != nullptr)) { set_error("keyframe_map_depth: Pose and Pos are given together (or both NULL)"); return EDGEHIP_ERR_ARG; }
    if (int e = kf_entry(c, slot_new, "keyframe_map_depth")) return e;
    const int e = kd_map_run(c, slot_new, Pose, Pos, reshape_q_abs, reshape_q_rel, location_uncertainty, out);
    const int r = slot_read_done(c, slot_new);
    return e ? e : r;
}

int edgehip_keyframe_translate_depth(edgehip_ctx *c, int slot_new, int direction, const double *Pose, const double *Pos, const double *K,
                                     int optim_scale, edgehip_kf_depth *out) {
    EH_ENTER(c);
    const char *who = "keyframe_translate_depth";
    if (direction != 0 && direction != 1) { set_error("keyframe_translate_depth: direction is 0 (frame -> key frame) or 1 (key frame -> frame)"); return EDGEHIP_ERR_ARG; }
    if (direction && optim_scale) { set_error("keyframe_translate_depth: optim_scale belongs to direction 0 (translateDepth_KF2F has no scale step)"); return EDGEHIP_ERR_ARG; }
    const int given = (Pose != nullptr) + (Pos != nullptr) + (K != nullptr);
    if (given != 0 && given != 3) { set_error("keyframe_translate_depth: Pose, Pos and K are given together (or all NULL)"); return EDGEHIP_ERR_ARG; }
    if (int e = kf_entry(c, slot_new, who)) return e;
    const int e = kd_translate_run(c, slot_new, direction, Pose, Pos, K, optim_scale != 0, out);
    const int r = slot_read_done(c, slot_new);
    return e ? e : r;
}

int edgehip_keyframe_list_translate_depth(edgehip_ctx *c, int iters, edgehip_kf_depth *out) {
    EH_ENTER(c);
    const char *who = "keyframe_list_translate_depth";
    auto *d = c->kftrack;
    if (!d) { set_error(std::string(who) + ": key-frame tracking is not enabled (edgehip_keyframe_track_enable)"); return EDGEHIP_ERR_STATE; }
    if (!d->list.hdr) { set_error(std::string(who) + ": the key-frame list is not enabled (edgehip_keyframe_list_enable)"); return EDGEHIP_ERR_STATE; }
    if (iters < 0) { set_error(std::string(who) + ": iters must be >= 0"); return EDGEHIP_ERR_ARG; }
    if (int e = kd_scratch(c, who)) return e;
    KdArgs a = kd_args(c, 0);
    if (int e = kd_begin(c)) return e;
    for (int it = 0; it < iters; it++) {
        a.count_on = it == iters - 1;
        for (a.pos = 0; a.pos < d->list.capacity; a.pos++) {   // ascending: position pos + 1 is still what the iteration began with
            hipLaunchKernelGGL(k_kd_rows<3>, kd_grid(c), dim3(kKdThreads), 0, c->stream, a);
            EH_LAUNCH_CHECK();
        }
    }
    if (int e = kd_end(c, out)) return e;
    if (!out) EH_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int edgehip_keyframe_depth_select(edgehip_ctx *c, const uint8_t *mask) {
    EH_ENTER(c);
    auto *d = c->kftrack;
    if (!d) { set_error("keyframe_depth_select: key-frame tracking is not enabled"); return EDGEHIP_ERR_STATE; }
    if (!mask) { d->kd_masked = false; return 0; }
    if (int e = kd_scratch(c, "keyframe_depth_select")) return e;
    EH_CHECK(hipMemcpyAsync(d->kd_mask_dev, mask, c->plan.nseq, hipMemcpyHostToDevice, c->stream));
    EH_CHECK(hipStreamSynchronize(c->stream));   // (the caller's array is free on return)
    d->kd_masked = true;
    return 0;
}

int edgehip_keyframe_depth_ms(edgehip_ctx *c, double *ms) {
    EH_ENTER(c);
    auto *d = c->kftrack;
    if (!d) { set_error("keyframe_depth_ms: key-frame tracking is not enabled"); return EDGEHIP_ERR_STATE; }
    float t = 0;
    if (d->kd_timed) {
        EH_CHECK(hipEventSynchronize(d->kd_ev[1]));
        EH_CHECK(hipEventElapsedTime(&t, d->kd_ev[0], d->kd_ev[1]));
    }
    if (ms) *ms = t;
    return 0;
}
