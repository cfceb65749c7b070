// keyframe_track.hip — the reference's TrackKeyFrames path (rebvo_second_t.cpp:156-162, 429-444, 587-598) for whole batches: a current key
// frame per sequence in HBM, and after every frame pair the repair of the matches between that key frame and the newest edge map in both
// directions — kfvo::buildForwardMatch, forwardCorrectAugmentate, correctAugmentate (src/mtracklib/kfvo.cpp:739-771, 969-1142, 804-966) —
// followed by the insertion rule.  Only m_id_f of the key frame's copy, m_id_kf of the frame lists and the counts change; nothing feeds
// back into the odometry.
//
// Both correctAugmentate functions have three phases.  Phase 1 (every matched KeyLine slides its match along the OTHER list's n_id / p_id
// chain while the epipolar distance strictly decreases) and phase 3 (matches whose phase-1 distance exceeds dist_thresh are dropped, the rest
// counted) are one thread per KeyLine.  Phase 2 is order dependent: for i ascending, a KeyLine that has a match at that moment walks its OWN
// list's p_id chain and then its n_id chain and hands its match to unmatched neighbours.  Its exact parallel form:
//   - a walk never leaves the connected component of its seed in the undirected graph of all p_id / n_id links of the own list, and the
//     other list is read-only in phase 2: work in different components commutes;
//   - components are labelled by their minimum index (atomic-min hooking + pointer jumping; the links are not mutual, several KeyLines may
//     share one n_id, cycles and self-links occur: edge_finder.cpp:304-320 — any link graph is handled);
//   - the keys (label << 16 | index) are sorted (bitonic), which lists every component's members in ascending index;
//   - one lane per component runs its members serially in that order, exactly as the reference's loop meets them.
// One workgroup per sequence does all of that; the label / key array of a sequence (4 B per KeyLine) sits in LDS up to 16384 KeyLines and
// in HBM above (EDGEHIP_KF_LDS=0: always HBM; DESIGN.md has the comparison).
//
// Arithmetic: E = R * crossMatrix(t) per sequence in the reference's operation order (TooN dot products accumulate in ascending index),
// fp64, no contraction (the Makefile's -ffp-contract=off), p_m widened from float as TooN::makeVector does.
//
// Preconditions (the reference has no defined result without them): finite p_m; m_id, m_id_f, m_id_kf in range of the lists they index or
// negative.  The device never reads out of bounds on other input: an out-of-range link ends a chain like a negative one, an out-of-range
// match is left alone with guard bit 2.  Every chain walk is capped at the length of the list it walks: on finite p_m a walk strictly
// decreases its distance and ends before that; a NaN p_m inside a link cycle (where the reference never returns) ends at the cap and sets
// guard bit 1.
#include "keyframe_track.h"
#include "link_components.h"

#include <cstdlib>
#include <type_traits>
#include <vector>

static_assert(EDGEHIP_KEYLINE_MAX <= 65536, "component keys pack (label, index) into 16 + 16 bits");

namespace edgehip {

constexpr int kKfThreads = 256;          // per-KeyLine kernels
constexpr int kKfAugThreads = 1024;      // phase 2: one workgroup per sequence
constexpr int kKfLdsKeys = 16384;        // keys that fit 64 KB of LDS

struct KfArgs {
    const KlSoA *slot_kl;    // [nseq] KeyLines of the frame slot
    const KlSoA *kf_kl;      // [nseq] the key frames
    const int32_t *slot_kn;  // [nseq]
    KfSeq *ks;               // [nseq]
    edgehip_kf_track *rec;   // [nseq]
    int32_t *table;          // [nseq][cap] buildForwardMatch's fowMatch
    double *dist;            // [nseq][cap]
    uint32_t *keys;          // [nseq][np2cap] labels, then keys (HBM form)
    int cap, np2cap, nseq;
    double thresh, tol, zfm;
    int dir;                 // 0: forward (own list = key frame, m_id_f), 1: back (own list = frame slot, m_id_kf)
    int augment, use_lds;
};

// One direction's view of the two lists.
struct KfView {
    const float2 *own_pm, *oth_pm;
    const int32_t *own_p, *own_n, *oth_p, *oth_n;
    int32_t *own_m;
    int own_kn, oth_kn;
    double E[9], zf;
};

__device__ __forceinline__ KfView kf_view(const KfArgs &a, int seq) {
    const KlSoA &s = a.slot_kl[seq], &k = a.kf_kl[seq];
    const int skn = max(0, min(a.slot_kn[seq], a.cap)), kkn = max(0, min(a.ks[seq].kn, a.cap));
    KfView v;
    const KlSoA &own = a.dir ? s : k, &oth = a.dir ? k : s;
    v.own_pm = own.p_m; v.own_p = own.p_id; v.own_n = own.n_id;
    v.oth_pm = oth.p_m; v.oth_p = oth.p_id; v.oth_n = oth.n_id;
    v.own_m = a.dir ? s.m_id_kf : k.m_id_f;
    v.own_kn = a.dir ? skn : kkn;
    v.oth_kn = a.dir ? kkn : skn;
    const double *E = a.dir ? a.ks[seq].Eb : a.ks[seq].Ef;
#pragma unroll
    for (int i = 0; i < 9; i++) v.E[i] = E[i];
    v.zf = a.zfm;
    return v;
}

// kfvo::forwardStereoCorrect / stereoCorrect (kfvo.cpp:1058-1142, 804-887) of a KeyLine at p_m with match f: the match slides along the
// other list's n_id chain, else its p_id chain, while the distance to the epipolar line strictly decreases.
__device__ double kf_slide(const KfView &v, const float2 pm, int &f, const double tol, int &guard) {
    if (f < 0) return -1;
    if (f >= v.oth_kn) { guard |= 2; return -1; }
    const double x = (double)pm.x, y = (double)pm.y;
    const double e0 = v.E[0] * x + v.E[1] * y + v.E[2] * v.zf;
    const double e1 = v.E[3] * x + v.E[4] * y + v.E[5] * v.zf;
    const double e2 = v.E[6] * x + v.E[7] * y + v.E[8] * v.zf;
    const double nrm = sqrt(e0 * e0 + e1 * e1);
    const double r0 = e0 / nrm, r1 = e1 / nrm, r2 = (e2 / nrm) * v.zf;
    auto dist_to = [&](int j) {
        const float2 q = ldg(v.oth_pm, j);
        return fabs((double)q.x * r0 + (double)q.y * r1 + r2);
    };
    auto link = [&](const int32_t *l, int j) {
        const int t = ldg(l, j);
        return t < v.oth_kn ? t : -1;
    };
    double d0 = dist_to(f);
    if (d0 < tol) return d0;
    int steps = 0;
    for (int side = 0; side < 2; side++) {
        const int32_t *l = side ? v.oth_p : v.oth_n;
        int nx = link(l, f);
        if (nx < 0) continue;
        double d = dist_to(nx);
        if (!(d < d0)) continue;
        while (1) {
            f = nx;
            d0 = d;
            if (d0 < tol) return d0;
            nx = link(l, f);
            if (nx < 0) return d0;
            d = dist_to(nx);
            if (d >= d0) return d0;
            if (++steps > v.oth_kn) { guard |= 1; return d0; }
        }
    }
    return d0;
}

// the second and third function of phase 2 (kfvo.cpp:998-1041, 923-966) for seed i
__device__ void kf_augment_seed(const KfView &v, const int i, const double thresh, const double tol, int &guard) {
    if (v.own_m[i] < 0) return;
    for (int side = 0; side < 2; side++) {
        const int32_t *l = side ? v.own_n : v.own_p;
        int kl = i, steps = 0;
        while (1) {
            const int j = ldg(l, kl);
            if (j < 0 || j >= v.own_kn) break;
            if (v.own_m[j] >= 0) break;
            int f = v.own_m[kl];
            const double d = kf_slide(v, ldg(v.own_pm, j), f, tol, guard);
            if (d > thresh) { v.own_m[j] = -1; break; }
            v.own_m[j] = f;
            kl = j;
            if (++steps > v.own_kn) { guard |= 1; break; }
        }
    }
}

// ---- per-sequence set-up: who runs, the two E matrices, the record's counters -------------------------------------------------------------
// mode 0: a stage-level entry (every sequence runs; Pose / Pos from `pose_in` [nseq][12] or, null, from seq_state); mode 1: the frame driver
// (sequences with klm_num >= MatchThreshold that got as far as matching; back_m0 = directed_matching's count).  clear: bit 0 fow_m0, bit 1
// fow_m, bit 2 back_m, bit 3 guard.
__device__ inline void kf_mat_tn(const double *A, const double *B, double *C) {   // C = A^T * B
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) C[r * 3 + c] = A[0 * 3 + r] * B[0 * 3 + c] + A[1 * 3 + r] * B[1 * 3 + c] + A[2 * 3 + r] * B[2 * 3 + c];
}
__device__ inline void kf_essential(const double *R, const double *t, double *E) {   // R * crossMatrix(t), products with the matrix's zeros included
    const double X[9] = {0, -t[2], t[1], t[2], 0, -t[0], -t[1], t[0], 0};
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) E[r * 3 + c] = R[r * 3 + 0] * X[0 * 3 + c] + R[r * 3 + 1] * X[1 * 3 + c] + R[r * 3 + 2] * X[2 * 3 + c];
}

__global__ void k_kf_setup(KfArgs a, const SeqDev *__restrict__ seqs, const double *__restrict__ pose_in, int mode, int match_threshold, int clear) {
    const int seq = blockIdx.x * blockDim.x + threadIdx.x;
    if (seq >= a.nseq) return;
    KfSeq &k = a.ks[seq];
    edgehip_kf_track &r = a.rec[seq];
    const edgehip_seq_state &p = seqs[seq].pub;
    int active = 1;
    if (mode == 1) {
        active = !seqs[seq].skip_match && p.klm_num >= match_threshold && k.kf_count > 0;
        r.back_m0 = p.kf_matchs;
        r.back_m = active ? 0 : p.kf_matchs;
        r.fow_m0 = 0; r.fow_m = 0;
    } else {
        if (clear & 1) r.fow_m0 = 0;
        if (clear & 2) r.fow_m = 0;
        if (clear & 4) r.back_m = 0;
    }
    if (clear & 8) r.guard = 0;
    k.active = active;
    if (!active) return;
    double Pose[9], Pos[3];
    if (pose_in) {
        for (int i = 0; i < 9; i++) Pose[i] = pose_in[(size_t)seq * 12 + i];
        for (int i = 0; i < 3; i++) Pos[i] = pose_in[(size_t)seq * 12 + 9 + i];
    } else {   // localPose = Pose * R, localPos = Pos - localPose * V * K (rebvo_second_t.cpp:435-436)
        for (int r_ = 0; r_ < 3; r_++)
            for (int c = 0; c < 3; c++) Pose[r_ * 3 + c] = p.Pose[r_ * 3 + 0] * p.R[0 * 3 + c] + p.Pose[r_ * 3 + 1] * p.R[1 * 3 + c] + p.Pose[r_ * 3 + 2] * p.R[2 * 3 + c];
        for (int i = 0; i < 3; i++) Pos[i] = p.Pos[i] - (Pose[i * 3 + 0] * p.V[0] + Pose[i * 3 + 1] * p.V[1] + Pose[i * 3 + 2] * p.V[2]) * p.K;
    }
    const double *KP = k.pose.Pose, *Kt = k.pose.Pos;
    double R[9], d[3], t[3], E[9];
    // forward (kfvo.cpp:972-974): R = Pose^T * kf.Pose, t = kf.Pose^T * (Pos - kf.Pos)
    kf_mat_tn(Pose, KP, R);
    for (int i = 0; i < 3; i++) d[i] = Pos[i] - Kt[i];
    for (int i = 0; i < 3; i++) t[i] = KP[0 * 3 + i] * d[0] + KP[1 * 3 + i] * d[1] + KP[2 * 3 + i] * d[2];
    kf_essential(R, t, E);
    for (int i = 0; i < 9; i++) k.Ef[i] = E[i];
    // back (kfvo.cpp:896-898): R = kf.Pose^T * Pose, t = Pose^T * (kf.Pos - Pos)
    kf_mat_tn(KP, Pose, R);
    for (int i = 0; i < 3; i++) d[i] = Kt[i] - Pos[i];
    for (int i = 0; i < 3; i++) t[i] = Pose[0 * 3 + i] * d[0] + Pose[1 * 3 + i] * d[1] + Pose[2 * 3 + i] * d[2];
    kf_essential(R, t, E);
    for (int i = 0; i < 9; i++) k.Eb[i] = E[i];
}

// ---- kfvo::buildForwardMatch (kfvo.cpp:739-771) ---------------------------------------------------------------------------------------
// fowMatch[new[i].m_id] = i for i ascending: the largest i wins — an atomic max on a table filled with -1.
__global__ __launch_bounds__(kKfThreads) void k_kf_fwd_scatter(KfArgs a) {
    const int seq = blockIdx.y, i = blockIdx.x * kKfThreads + threadIdx.x;
    if (!a.ks[seq].active) return;
    const int kn = max(0, min(a.slot_kn[seq], a.cap));
    if (i >= kn) return;
    const int m = ldg(a.slot_kl[seq].m_id, i);
    if (m >= 0 && m < a.cap) atomicMax(a.table + (size_t)seq * a.cap + m, i);
}
__global__ __launch_bounds__(kKfThreads) void k_kf_fwd_repoint(KfArgs a) {
    const int seq = blockIdx.y, i = blockIdx.x * kKfThreads + threadIdx.x;
    if (!a.ks[seq].active) return;
    const int kn = max(0, min(a.ks[seq].kn, a.cap));
    int hit = 0;
    if (i < kn) {
        int32_t *mf = a.kf_kl[seq].m_id_f;
        const int f = mf[i];
        if (f >= 0) {
            const int nm = f < a.cap ? a.table[(size_t)seq * a.cap + f] : -1;
            mf[i] = nm < 0 ? -1 : nm;
            hit = nm >= 0;
        }
    }
    const int n = __syncthreads_count(hit);
    if (threadIdx.x == 0 && n) atomicAdd(&a.rec[seq].fow_m0, n);
}

// ---- phase 1 and phase 3 --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kKfThreads) void k_kf_phase1(KfArgs a) {
    const int seq = blockIdx.y, i = blockIdx.x * kKfThreads + threadIdx.x;
    if (!a.ks[seq].active) return;
    const KfView v = kf_view(a, seq);
    if (i >= v.own_kn) return;
    int f = v.own_m[i], guard = 0;
    const double d = kf_slide(v, ldg(v.own_pm, i), f, a.tol, guard);
    v.own_m[i] = f;
    a.dist[(size_t)seq * a.cap + i] = d;
    if (guard) atomicOr(&a.rec[seq].guard, guard);
}
__global__ __launch_bounds__(kKfThreads) void k_kf_phase3(KfArgs a) {
    const int seq = blockIdx.y, i = blockIdx.x * kKfThreads + threadIdx.x;
    if (!a.ks[seq].active) return;
    const KfView v = kf_view(a, seq);
    int hit = 0;
    if (i < v.own_kn) {
        if (a.dist[(size_t)seq * a.cap + i] > a.thresh) v.own_m[i] = -1;
        hit = v.own_m[i] >= 0;
    }
    const int n = __syncthreads_count(hit);
    if (threadIdx.x == 0 && n) atomicAdd(a.dir ? &a.rec[seq].back_m : &a.rec[seq].fow_m, n);
}
// the repaired back count is what SecondThread keeps in num_kf_back_m: the nav record's kf_matchs
__global__ void k_kf_finish(KfArgs a, SeqDev *seqs) {
    const int seq = blockIdx.x * blockDim.x + threadIdx.x;
    if (seq >= a.nseq || !a.ks[seq].active) return;
    seqs[seq].pub.kf_matchs = a.rec[seq].back_m;
}

// ---- phase 2 ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kKfAugThreads) void k_kf_augment(KfArgs a) {
    extern __shared__ uint32_t kf_lds[];
    __shared__ int changed;
    const int seq = blockIdx.x, tid = threadIdx.x;
    if (!a.ks[seq].active) return;   // block-uniform
    const KfView v = kf_view(a, seq);
    const int kn = v.own_kn;
    if (kn <= 0) return;
    int np2 = 1;
    while (np2 < kn) np2 <<= 1;
    uint32_t *buf = (a.use_lds && np2 <= kKfLdsKeys) ? kf_lds : a.keys + (size_t)seq * a.np2cap;
    // 1. components of the own list's undirected link graph, labelled by their minimum index (link_components.h)
    lc_label_min<kKfAugThreads, 2>(buf, kn, &changed, [&](int i, int side) { return ldg(side ? v.own_n : v.own_p, i); });
    // 2. keys (label, index), sorted: every component's members in ascending index, components one after the other.  Only members that can
    // act get a key: a seed acts only where one of its links names a KeyLine that is unmatched at that moment, and during phase 2 a
    // KeyLine never goes from matched to unmatched (a failed correction writes -1 over a negative value) — so a member none of whose links
    // names a KeyLine unmatched NOW walks nowhere whenever its turn comes, and leaving it out changes nothing.  After a few frames nine
    // members in ten go this way, and the serial lanes below are what the kernel's time is made of.
    for (int i = tid; i < np2; i += kKfAugThreads) {
        uint32_t key = 0xFFFFFFFFu;
        if (i < kn) {
            const int jp = ldg(v.own_p, i), jn = ldg(v.own_n, i);
            const bool acts = (jp >= 0 && jp < kn && v.own_m[jp] < 0) || (jn >= 0 && jn < kn && v.own_m[jn] < 0);
            if (acts) key = buf[i] << 16 | (uint32_t)i;
        }
        buf[i] = key;
    }
    __syncthreads();
    lc_sort<kKfAugThreads>(buf, np2);
    // 3. one lane per component, its members as seeds in ascending index
    int guard = 0;
    for (int k = tid; k < kn; k += kKfAugThreads) {
        const uint32_t key = buf[k];
        if (key == 0xFFFFFFFFu) break;   // (sorted: only members without a key from here on)
        const uint32_t lab = key >> 16;
        if (k > 0 && (buf[k - 1] >> 16) == lab) continue;
        for (int q = k; q < kn && (buf[q] >> 16) == lab; q++) kf_augment_seed(v, (int)(buf[q] & 0xFFFFu), a.thresh, a.tol, guard);
    }
    if (guard) atomicOr(&a.rec[seq].guard, guard);
}

// ---- insertion (keyframe.cpp:28-43) and the two resets (kfvo.cpp:774-787) -----------------------------------------------------------------
// mode 0: the sequences of `mask` (null: all), pose block from `pose_in` or, null, from the frame's nav record and seq_state.K;
// mode 1: sequences without a key frame (rebvo_second_t.cpp:156-162: K = 1, the old frame's nav record);
// mode 2: sequences whose repaired back count fell below min(TrackPoints, KNum) * KFSavePercent (:591-596).
// With the key-frame list on (list.hdr), the header of a key frame that is about to be replaced goes into the list here, where its pose
// block, kn and ordinal are last seen; k_kf_retire (keyframe_list.hip) takes its records before k_kf_copy runs.
__global__ void k_kf_decide(KfArgs a, const SeqDev *__restrict__ seqs, const edgehip_nav *__restrict__ nav, const uint8_t *__restrict__ mask,
                            const edgehip_kf_pose *__restrict__ pose_in, int mode, int track_points, double save_percent, int save_keyframes,
                            KfListDev list) {
    const int seq = blockIdx.x * blockDim.x + threadIdx.x;
    if (seq >= a.nseq) return;
    KfSeq &k = a.ks[seq];
    edgehip_kf_track &r = a.rec[seq];
    const int kn = max(0, min(a.slot_kn[seq], a.cap));
    int ins;
    if (mode == 0) ins = mask ? mask[seq] != 0 : 1;
    else if (mode == 1) ins = k.kf_count == 0;
    else ins = save_keyframes && k.kf_count > 0 && (double)seqs[seq].pub.kf_matchs < (double)min(track_points, kn) * save_percent;
    k.do_insert = ins;
    if (mode == 1) r.inserted = ins;
    else if (ins) r.inserted = 1;
    if (list.hdr) kf_list_retire_head(list, seq, k, ins != 0);
    if (ins) {
        if (pose_in) {
            k.pose = pose_in[seq];
        } else {
            const edgehip_nav &o = nav[seq];
            edgehip_kf_pose q;
            q.t = o.t;
            q.K = mode == 1 ? 1.0 : seqs[seq].pub.K;
            for (int i = 0; i < 9; i++) { q.Rot[i] = o.Rot[i]; q.Pose[i] = o.Pose[i]; }
            for (int i = 0; i < 3; i++) { q.RotLie[i] = o.RotLie[i]; q.Vel[i] = o.Vel[i]; q.PoseLie[i] = o.PoseLie[i]; q.Pos[i] = o.Pos[i]; }
            k.pose = q;
        }
        k.kn = kn;
        k.kf_count++;
    }
    r.kf_count = k.kf_count;
    r.kf_kn = k.kn;
}

__global__ __launch_bounds__(kKfThreads) void k_kf_copy(KfArgs a) {
    const int seq = blockIdx.y, i = blockIdx.x * kKfThreads + threadIdx.x;
    if (!a.ks[seq].do_insert) return;
    const int kn = max(0, min(a.slot_kn[seq], a.cap));
    if (i >= kn) return;
    const KlSoA &s = a.slot_kl[seq], &k = a.kf_kl[seq];
    k.p_inx[i] = s.p_inx[i];
    k.m_m[i] = s.m_m[i]; k.u_m[i] = s.u_m[i]; k.c_p[i] = s.c_p[i]; k.p_m[i] = s.p_m[i]; k.p_m_0[i] = s.p_m_0[i]; k.m_m0[i] = s.m_m0[i];
    k.n_m[i] = s.n_m[i];
    const double rho = s.rho[i], s_rho = s.s_rho[i];
    k.rho[i] = rho; k.s_rho[i] = s_rho; k.rho_nr[i] = s.rho_nr[i]; k.s_rho_nr[i] = s.s_rho_nr[i];
    k.rho0[i] = rho; k.s_rho0[i] = s_rho;          // resetForwardMatch
    k.n_m0[i] = s.n_m0[i];
    k.m_id[i] = s.m_id[i]; k.m_num[i] = s.m_num[i]; k.p_id[i] = s.p_id[i]; k.n_id[i] = s.n_id[i];
    k.m_id_f[i] = i;                               // resetForwardMatch
    k.m_id_kf[i] = s.m_id_kf[i];                   // (the copy is taken before resetKFMatch touches the frame's list)
    s.m_id_kf[i] = i;                              // resetKFMatch
    if (s.stereo_m_id) { k.stereo_m_id[i] = s.stereo_m_id[i]; k.stereo_rho[i] = s.stereo_rho[i]; k.stereo_s_rho[i] = s.stereo_s_rho[i]; }
}

// ---- the 168-byte records of a key frame <-> its arrays (upload / download) ------------------------------------------------------------
__global__ __launch_bounds__(kKfThreads) void k_kf_pack(KlSoA k, int kn, edgehip_keyline *__restrict__ out) {
    const int i = blockIdx.x * kKfThreads + threadIdx.x;
    if (i >= kn) return;
    edgehip_keyline o = {};
    o.p_inx = k.p_inx[i];
    const float2 m_m = k.m_m[i], u_m = k.u_m[i], c_p = k.c_p[i], p_m = k.p_m[i], p_m_0 = k.p_m_0[i], m_m0 = k.m_m0[i];
    o.m_m[0] = m_m.x; o.m_m[1] = m_m.y; o.u_m[0] = u_m.x; o.u_m[1] = u_m.y;
    o.n_m = k.n_m[i]; o.score = 0.f;
    o.c_p[0] = c_p.x; o.c_p[1] = c_p.y;
    o.rho = k.rho[i]; o.s_rho = k.s_rho[i]; o.rho_nr = k.rho_nr[i]; o.s_rho_nr = k.s_rho_nr[i]; o.rho0 = k.rho0[i]; o.s_rho0 = k.s_rho0[i];
    o.p_m[0] = p_m.x; o.p_m[1] = p_m.y; o.p_m_0[0] = p_m_0.x; o.p_m_0[1] = p_m_0.y;
    o.m_id = k.m_id[i]; o.m_id_f = k.m_id_f[i]; o.m_id_kf = k.m_id_kf[i]; o.m_num = k.m_num[i];
    o.m_m0[0] = m_m0.x; o.m_m0[1] = m_m0.y; o.n_m0 = k.n_m0[i];
    o.p_id = k.p_id[i]; o.n_id = k.n_id[i];
    o.net_id = -1; o.stereo_m_id = -1; o.stereo_rho = 1.0; o.stereo_s_rho = 20.0;   // what edgehip_download_keylines gives the fields the device does not keep
    if (k.stereo_m_id) { o.stereo_m_id = k.stereo_m_id[i]; o.stereo_rho = k.stereo_rho[i]; o.stereo_s_rho = k.stereo_s_rho[i]; }
    out[i] = o;
}
__global__ __launch_bounds__(kKfThreads) void k_kf_unpack(KlSoA k, int kn, const edgehip_keyline *__restrict__ in) {
    const int i = blockIdx.x * kKfThreads + threadIdx.x;
    if (i >= kn) return;
    const edgehip_keyline o = in[i];
    k.p_inx[i] = o.p_inx;
    k.m_m[i] = make_float2(o.m_m[0], o.m_m[1]); k.u_m[i] = make_float2(o.u_m[0], o.u_m[1]); k.c_p[i] = make_float2(o.c_p[0], o.c_p[1]);
    k.p_m[i] = make_float2(o.p_m[0], o.p_m[1]); k.p_m_0[i] = make_float2(o.p_m_0[0], o.p_m_0[1]); k.m_m0[i] = make_float2(o.m_m0[0], o.m_m0[1]);
    k.n_m[i] = o.n_m;
    k.rho[i] = o.rho; k.s_rho[i] = o.s_rho; k.rho_nr[i] = o.rho_nr; k.s_rho_nr[i] = o.s_rho_nr; k.rho0[i] = o.rho0; k.s_rho0[i] = o.s_rho0;
    k.n_m0[i] = o.n_m0;
    k.m_id[i] = o.m_id; k.m_id_f[i] = o.m_id_f; k.m_id_kf[i] = o.m_id_kf; k.m_num[i] = o.m_num; k.p_id[i] = o.p_id; k.n_id[i] = o.n_id;
    if (k.stereo_m_id) { k.stereo_m_id[i] = o.stereo_m_id; k.stereo_rho[i] = o.stereo_rho; k.stereo_s_rho[i] = o.stereo_s_rho; }
}

}  // namespace edgehip

using namespace edgehip;

void edgehip::kf_track_free(edgehip_ctx *c) {
    auto *d = c->kftrack;
    if (!d) return;
    (void)hipStreamSynchronize(c->stream);
    kf_list_free(c);
    kf_covis_free(c);
    kf_reloc_free(c);
    kf_constraint_free(c);
    kf_depth_free(c);
    for (void *q : d->dev) (void)hipFree(q);
    if (d->pose12_host) (void)hipHostFree(d->pose12_host);
    if (d->blk_host) (void)hipHostFree(d->blk_host);
    if (d->mask_host) (void)hipHostFree(d->mask_host);
    if (d->ev) (void)hipEventDestroy(d->ev);
    delete d;
    c->kftrack = nullptr;
}

template <class T> static bool kf_alloc(edgehip_ctx::KfTrack *d, T **p, size_t count) {
    void *q = nullptr;
    if (hipMalloc(&q, sizeof(T) * std::max<size_t>(count, 1)) != hipSuccess) { (void)hipGetLastError(); return false; }
    d->dev.push_back(q);
    *p = (T *)q;
    return true;
}

int edgehip_keyframe_track_enable(edgehip_ctx *c, int enable, double kf_save_percent, int save_keyframes) {
    EH_ENTER(c);
    if (enable && c->imu_enabled) { set_error("keyframe_track_enable: the device IMU branch does not track key frames"); return EDGEHIP_ERR_STATE; }
    if (enable < 0 || enable > 2) { set_error("keyframe_track_enable: enable is 0, 1 or 2"); return EDGEHIP_ERR_ARG; }
    if (enable && !(kf_save_percent >= 0)) { set_error("keyframe_track_enable: KFSavePercent must be >= 0"); return EDGEHIP_ERR_ARG; }
    drop_frame_graphs(c);   // a captured frame enqueues what the feature's state said when it was captured
    kf_track_free(c);
    if (!enable) return 0;
    // 64 KB of keys beside the kernel's own few bytes of LDS: opt in (the attribute belongs to the kernel, setting it again is harmless)
    EH_CHECK(hipFuncSetAttribute((const void *)&k_kf_augment, hipFuncAttributeMaxDynamicSharedMemorySize, kKfLdsKeys * (int)sizeof(uint32_t)));
    auto *d = c->kftrack = new edgehip_ctx::KfTrack;
    const size_t B = c->plan.nseq, CAP = c->plan.cap;
    d->save_percent = kf_save_percent;
    d->save_keyframes = save_keyframes != 0;
    d->in_driver = enable == 1;
    d->use_lds = getenv("EDGEHIP_KF_LDS") ? atoi(getenv("EDGEHIP_KF_LDS")) != 0 : 1;
    while ((size_t)d->np2cap < CAP) d->np2cap <<= 1;
    const bool stereo = klof(c, 0, 0).stereo_m_id != nullptr;
    d->kl.assign(B, KlSoA());
    bool ok = true;
    // the key frames' arrays: one allocation per field, [nseq][cap]
    auto field = [&](auto KlSoA::*m) {
        typename std::remove_pointer<typename std::remove_reference<decltype(d->kl[0].*m)>::type>::type *base = nullptr;
        ok = ok && kf_alloc(d, &base, B * CAP);
        if (ok) for (size_t s = 0; s < B; s++) d->kl[s].*m = base + s * CAP;
    };
    field(&KlSoA::p_inx); field(&KlSoA::m_m); field(&KlSoA::u_m); field(&KlSoA::c_p); field(&KlSoA::p_m); field(&KlSoA::p_m_0); field(&KlSoA::m_m0);
    field(&KlSoA::n_m); field(&KlSoA::rho); field(&KlSoA::s_rho); field(&KlSoA::rho_nr); field(&KlSoA::s_rho_nr); field(&KlSoA::rho0);
    field(&KlSoA::s_rho0); field(&KlSoA::n_m0); field(&KlSoA::m_id); field(&KlSoA::m_id_f); field(&KlSoA::m_id_kf); field(&KlSoA::m_num);
    field(&KlSoA::p_id); field(&KlSoA::n_id);
    if (stereo) { field(&KlSoA::stereo_m_id); field(&KlSoA::stereo_rho); field(&KlSoA::stereo_s_rho); }
    ok = ok && kf_alloc(d, &d->kl_dev, B) && kf_alloc(d, &d->ks, B) && kf_alloc(d, &d->rec, B) && kf_alloc(d, &d->table, B * CAP) &&
         kf_alloc(d, &d->dist, B * CAP) && kf_alloc(d, &d->keys, B * (size_t)d->np2cap) && kf_alloc(d, &d->aos, CAP) &&
         kf_alloc(d, &d->pose12_dev, B * 12) && kf_alloc(d, &d->blk_dev, B) && kf_alloc(d, &d->mask_dev, B) &&
         kf_alloc(d, &d->kc_counts, B * 2);
    ok = ok && hipHostMalloc((void **)&d->pose12_host, 8 * 12 * B, hipHostMallocDefault) == hipSuccess &&
         hipHostMalloc((void **)&d->blk_host, sizeof(edgehip_kf_pose) * B, hipHostMallocDefault) == hipSuccess &&
         hipHostMalloc((void **)&d->mask_host, B, hipHostMallocDefault) == hipSuccess &&
         hipEventCreateWithFlags(&d->ev, hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        kf_track_free(c);
        set_error("keyframe_track_enable: allocation failed");
        return EDGEHIP_ERR_MEMORY;
    }
    hipError_t e = hipMemcpyAsync(d->kl_dev, d->kl.data(), sizeof(KlSoA) * B, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d->ks, 0, sizeof(KfSeq) * B, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d->rec, 0, sizeof(edgehip_kf_track) * B, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d->aos, 0, sizeof(edgehip_keyline) * CAP, c->stream);   // (the records' padding never carries stale device memory)
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // (d->kl is read by the copy above)
    if (e != hipSuccess) kf_track_free(c);
    EH_CHECK(e);
    return 0;
}

int edgehip::kf_track_reset_enqueue(edgehip_ctx *c) {
    auto *d = c->kftrack;
    if (!d) return 0;
    EH_CHECK(hipMemsetAsync(d->ks, 0, sizeof(KfSeq) * c->plan.nseq, c->stream));
    EH_CHECK(hipMemsetAsync(d->rec, 0, sizeof(edgehip_kf_track) * c->plan.nseq, c->stream));
    return kf_list_reset_enqueue(c);
}

static KfArgs kf_args(edgehip_ctx *c, int slot) {
    auto *d = c->kftrack;
    KfArgs a;
    a.slot_kl = kldev(c, slot);
    a.kf_kl = d->kl_dev;
    a.slot_kn = c->kn_slot + (size_t)slot * c->plan.nseq;
    a.ks = d->ks; a.rec = d->rec; a.table = d->table; a.dist = d->dist; a.keys = d->keys;
    a.cap = c->plan.cap; a.np2cap = d->np2cap; a.nseq = c->plan.nseq;
    a.thresh = 10; a.tol = 0; a.zfm = c->plan.zfm;
    a.dir = 0; a.augment = 1; a.use_lds = d->use_lds;
    return a;
}
static dim3 kf_grid(edgehip_ctx *c) { return dim3((c->plan.cap + kKfThreads - 1) / kKfThreads, c->plan.nseq); }
static dim3 kf_seq_grid(edgehip_ctx *c) { return dim3((c->plan.nseq + 63) / 64); }

// the page-locked rows are free again once the last copy out of them has run
static int kf_stage_wait(edgehip_ctx::KfTrack *d) {
    if (d->busy) EH_CHECK(hipEventSynchronize(d->ev));
    d->busy = false;
    return 0;
}
static int kf_stage_posted(edgehip_ctx *c) {
    EH_CHECK(hipEventRecord(c->kftrack->ev, c->stream));
    c->kftrack->busy = true;
    return 0;
}

static int kf_build_forward_enqueue(edgehip_ctx *c, const KfArgs &a) {
    EH_CHECK(hipMemsetAsync(a.table, 0xFF, sizeof(int32_t) * (size_t)a.nseq * a.cap, c->stream));
    hipLaunchKernelGGL(k_kf_fwd_scatter, kf_grid(c), dim3(kKfThreads), 0, c->stream, a);
    EH_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_kf_fwd_repoint, kf_grid(c), dim3(kKfThreads), 0, c->stream, a);
    EH_LAUNCH_CHECK();
    return 0;
}
static int kf_correct_enqueue(edgehip_ctx *c, KfArgs a, int dir) {
    a.dir = dir;
    hipLaunchKernelGGL(k_kf_phase1, kf_grid(c), dim3(kKfThreads), 0, c->stream, a);
    EH_LAUNCH_CHECK();
    if (a.augment) {
        const size_t lds = a.use_lds ? sizeof(uint32_t) * (size_t)std::min(a.np2cap, kKfLdsKeys) : 0;
        hipLaunchKernelGGL(k_kf_augment, dim3(a.nseq), dim3(kKfAugThreads), lds, c->stream, a);
        EH_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_kf_phase3, kf_grid(c), dim3(kKfThreads), 0, c->stream, a);
    EH_LAUNCH_CHECK();
    return 0;
}

// ---- the frame driver's three hooks (stage_c.hip: frame_enqueue) ------------------------------------------------------------------------
int edgehip::kf_frame_begin_enqueue(edgehip_ctx *c, int slot_old) {   // rebvo_second_t.cpp:156-162
    if (!c->kftrack->in_driver) return 0;
    KfArgs a = kf_args(c, slot_old);
    hipLaunchKernelGGL(k_kf_decide, kf_seq_grid(c), dim3(64), 0, c->stream, a, (const SeqDev *)c->seq, (const edgehip_nav *)c->nav_dev,
                       (const uint8_t *)nullptr, (const edgehip_kf_pose *)nullptr, 1, 0, 0.0, 0, c->kftrack->list);
    EH_LAUNCH_CHECK();
    if (int e = kf_list_retire_enqueue(c)) return e;
    hipLaunchKernelGGL(k_kf_copy, kf_grid(c), dim3(kKfThreads), 0, c->stream, a);
    EH_LAUNCH_CHECK();
    return 0;
}
int edgehip::kf_frame_track_enqueue(edgehip_ctx *c, int slot_new) {   // :429-444
    if (!c->kftrack->in_driver) return 0;
    KfArgs a = kf_args(c, slot_new);
    hipLaunchKernelGGL(k_kf_setup, kf_seq_grid(c), dim3(64), 0, c->stream, a, (const SeqDev *)c->seq, (const double *)nullptr, 1,
                       c->p.global_match_threshold, 8);
    EH_LAUNCH_CHECK();
    if (int e = kf_build_forward_enqueue(c, a)) return e;
    if (int e = kf_correct_enqueue(c, a, 0)) return e;
    if (int e = kf_correct_enqueue(c, a, 1)) return e;
    hipLaunchKernelGGL(k_kf_finish, kf_seq_grid(c), dim3(64), 0, c->stream, a, c->seq);
    EH_LAUNCH_CHECK();
    return 0;
}
int edgehip::kf_frame_end_enqueue(edgehip_ctx *c, int slot_new) {   // :591-596
    if (!c->kftrack->in_driver) return 0;
    auto *d = c->kftrack;
    KfArgs a = kf_args(c, slot_new);
    hipLaunchKernelGGL(k_kf_decide, kf_seq_grid(c), dim3(64), 0, c->stream, a, (const SeqDev *)c->seq, (const edgehip_nav *)c->nav_dev,
                       (const uint8_t *)nullptr, (const edgehip_kf_pose *)nullptr, 2, c->p.track_points, d->save_percent, d->save_keyframes, d->list);
    EH_LAUNCH_CHECK();
    if (int e = kf_list_retire_enqueue(c)) return e;
    hipLaunchKernelGGL(k_kf_copy, kf_grid(c), dim3(kKfThreads), 0, c->stream, a);
    EH_LAUNCH_CHECK();
    return 0;
}

// ---- stage-level entry points ---------------------------------------------------------------------------------------------------------
int edgehip::kf_entry(edgehip_ctx *c, int slot, const char *who) {
    if (!c->kftrack) { set_error(std::string(who) + ": key-frame tracking is not enabled (edgehip_keyframe_track_enable)"); return EDGEHIP_ERR_STATE; }
    if (slot < 0 || slot >= c->plan.nslots) { set_error(std::string(who) + ": slot out of range"); return EDGEHIP_ERR_ARG; }
    if (int e = rot_materialize_enqueue(c, slot)) return e;   // the slot's KeyLines as edgehip_download_keylines returns them
    return order_bc_after_a(c);
}
// counts[nseq] <- one int32 field of the records.  Synchronises.
static int kf_counts_out(edgehip_ctx *c, size_t field_off, int32_t *counts) {
    if (!counts) return 0;
    std::vector<edgehip_kf_track> r(c->plan.nseq);
    EH_CHECK(hipMemcpyAsync(r.data(), c->kftrack->rec, sizeof(edgehip_kf_track) * r.size(), hipMemcpyDeviceToHost, c->stream));
    EH_CHECK(hipStreamSynchronize(c->stream));
    for (size_t s = 0; s < r.size(); s++) counts[s] = *(const int32_t *)((const char *)&r[s] + field_off);
    return 0;
}

int edgehip_keyframe_insert(edgehip_ctx *c, int slot, const uint8_t *mask, const edgehip_kf_pose *pose) {
    EH_ENTER(c);
    if (int e = kf_entry(c, slot, "keyframe_insert")) return e;
    auto *d = c->kftrack;
    const size_t B = c->plan.nseq;
    if (mask || pose) {
        if (int e = kf_stage_wait(d)) return e;
        if (mask) { memcpy(d->mask_host, mask, B); EH_CHECK(hipMemcpyAsync(d->mask_dev, d->mask_host, B, hipMemcpyHostToDevice, c->stream)); }
        if (pose) { memcpy(d->blk_host, pose, sizeof(edgehip_kf_pose) * B); EH_CHECK(hipMemcpyAsync(d->blk_dev, d->blk_host, sizeof(edgehip_kf_pose) * B, hipMemcpyHostToDevice, c->stream)); }
        if (int e = kf_stage_posted(c)) return e;
    }
    KfArgs a = kf_args(c, slot);
    hipLaunchKernelGGL(k_kf_decide, kf_seq_grid(c), dim3(64), 0, c->stream, a, (const SeqDev *)c->seq, (const edgehip_nav *)c->nav_dev,
                       (const uint8_t *)(mask ? d->mask_dev : nullptr), (const edgehip_kf_pose *)(pose ? d->blk_dev : nullptr), 0, 0, 0.0, 0, d->list);
    EH_LAUNCH_CHECK();
    if (int e = kf_list_retire_enqueue(c)) return e;
    hipLaunchKernelGGL(k_kf_copy, kf_grid(c), dim3(kKfThreads), 0, c->stream, a);
    EH_LAUNCH_CHECK();
    return slot_read_done(c, slot);
}

// Pose[nseq][9] | Pos[nseq][3] -> the device's [nseq][12] rows; both null: the kernel takes them from seq_state
static int kf_push_pose(edgehip_ctx *c, const double *Pose, const double *Pos, const double **dev_out) {
    auto *d = c->kftrack;
    *dev_out = nullptr;
    if (!Pose && !Pos) return 0;
    if (!Pose || !Pos) { set_error("keyframe tracking: Pose and Pos are given together (or both NULL)"); return EDGEHIP_ERR_ARG; }
    if (int e = kf_stage_wait(d)) return e;
    for (int s = 0; s < c->plan.nseq; s++) {
        memcpy(d->pose12_host + (size_t)s * 12, Pose + (size_t)s * 9, 72);
        memcpy(d->pose12_host + (size_t)s * 12 + 9, Pos + (size_t)s * 3, 24);
    }
    EH_CHECK(hipMemcpyAsync(d->pose12_dev, d->pose12_host, 96 * (size_t)c->plan.nseq, hipMemcpyHostToDevice, c->stream));
    if (int e = kf_stage_posted(c)) return e;
    *dev_out = d->pose12_dev;
    return 0;
}

int edgehip_keyframe_build_forward_match(edgehip_ctx *c, int slot_new, int32_t *counts) {
    EH_ENTER(c);
    if (int e = kf_entry(c, slot_new, "keyframe_build_forward_match")) return e;
    KfArgs a = kf_args(c, slot_new);
    hipLaunchKernelGGL(k_kf_setup, kf_seq_grid(c), dim3(64), 0, c->stream, a, (const SeqDev *)c->seq, (const double *)nullptr, 0, 0, 1);
    EH_LAUNCH_CHECK();
    if (int e = kf_build_forward_enqueue(c, a)) return e;
    if (int e = slot_read_done(c, slot_new)) return e;
    return kf_counts_out(c, offsetof(edgehip_kf_track, fow_m0), counts);
}

static int kf_correct_entry(edgehip_ctx *c, int slot_new, const double *Pose, const double *Pos, double dist_thresh, double dist_tolerance,
                            int augmentate, int32_t *counts, int dir, const char *who) {
    if (int e = kf_entry(c, slot_new, who)) return e;
    const double *pose_dev = nullptr;
    if (int e = kf_push_pose(c, Pose, Pos, &pose_dev)) return e;
    KfArgs a = kf_args(c, slot_new);
    a.thresh = dist_thresh; a.tol = dist_tolerance; a.augment = augmentate != 0;
    hipLaunchKernelGGL(k_kf_setup, kf_seq_grid(c), dim3(64), 0, c->stream, a, (const SeqDev *)c->seq, pose_dev, 0, 0, (dir ? 4 : 2) | 8);
    EH_LAUNCH_CHECK();
    if (int e = kf_correct_enqueue(c, a, dir)) return e;
    if (int e = slot_read_done(c, slot_new)) return e;
    return kf_counts_out(c, dir ? offsetof(edgehip_kf_track, back_m) : offsetof(edgehip_kf_track, fow_m), counts);
}
int edgehip_keyframe_forward_correct(edgehip_ctx *c, int slot_new, const double *Pose, const double *Pos, double dist_thresh,
                                     double dist_tolerance, int augmentate, int32_t *counts) {
    EH_ENTER(c);
    return kf_correct_entry(c, slot_new, Pose, Pos, dist_thresh, dist_tolerance, augmentate, counts, 0, "keyframe_forward_correct");
}
int edgehip_keyframe_back_correct(edgehip_ctx *c, int slot_new, const double *Pose, const double *Pos, double dist_thresh,
                                  double dist_tolerance, int augmentate, int32_t *counts) {
    EH_ENTER(c);
    return kf_correct_entry(c, slot_new, Pose, Pos, dist_thresh, dist_tolerance, augmentate, counts, 1, "keyframe_back_correct");
}

int edgehip_read_keyframe_track(edgehip_ctx *c, edgehip_kf_track *out) {
    EH_ENTER(c);
    if (!out) return EDGEHIP_ERR_ARG;
    if (!c->kftrack) { set_error("read_keyframe_track: key-frame tracking is not enabled"); return EDGEHIP_ERR_STATE; }
    EH_CHECK(hipMemcpyAsync(out, c->kftrack->rec, sizeof(edgehip_kf_track) * c->plan.nseq, hipMemcpyDeviceToHost, c->stream));
    EH_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int edgehip_download_keyframe(edgehip_ctx *c, int seq, edgehip_keyline *kl, int32_t *kn_out, edgehip_kf_pose *pose, int32_t *kf_count) {
    EH_ENTER(c);
    auto *d = c->kftrack;
    if (!d) { set_error("download_keyframe: key-frame tracking is not enabled"); return EDGEHIP_ERR_STATE; }
    if (seq < 0 || seq >= c->plan.nseq) { set_error("download_keyframe: sequence out of range"); return EDGEHIP_ERR_ARG; }
    KfSeq k;
    EH_CHECK(hipMemcpyAsync(&k, d->ks + seq, sizeof k, hipMemcpyDeviceToHost, c->stream));
    EH_CHECK(hipStreamSynchronize(c->stream));
    const int kn = std::max(0, std::min(k.kn, c->plan.cap));
    if (kl && kn > 0) {
        hipLaunchKernelGGL(k_kf_pack, dim3((kn + kKfThreads - 1) / kKfThreads), dim3(kKfThreads), 0, c->stream, d->kl[seq], kn, d->aos);
        EH_LAUNCH_CHECK();
        EH_CHECK(hipMemcpyAsync(kl, d->aos, sizeof(edgehip_keyline) * kn, hipMemcpyDeviceToHost, c->stream));
        EH_CHECK(hipStreamSynchronize(c->stream));
    }
    if (kn_out) *kn_out = kn;
    if (pose) *pose = k.pose;
    if (kf_count) *kf_count = k.kf_count;
    return 0;
}

int edgehip_upload_keyframe(edgehip_ctx *c, int seq, const edgehip_keyline *kl, int32_t kn, const edgehip_kf_pose *pose) {
    EH_ENTER(c);
    auto *d = c->kftrack;
    if (!d) { set_error("upload_keyframe: key-frame tracking is not enabled"); return EDGEHIP_ERR_STATE; }
    if (seq < 0 || seq >= c->plan.nseq) { set_error("upload_keyframe: sequence out of range"); return EDGEHIP_ERR_ARG; }
    if (kn < 0 || kn > c->plan.cap || (kn > 0 && !kl) || !pose) { set_error("upload_keyframe: kn exceeds max_points, or a null pointer"); return EDGEHIP_ERR_ARG; }
    KfSeq k;
    EH_CHECK(hipMemcpyAsync(&k, d->ks + seq, sizeof k, hipMemcpyDeviceToHost, c->stream));
    EH_CHECK(hipStreamSynchronize(c->stream));
    if (int e = kf_list_retire_one_enqueue(c, seq)) return e;   // the outgoing key frame into the list, before its arrays are overwritten
    k.pose = *pose;
    k.kn = kn;
    k.kf_count++;
    if (kn > 0) {
        EH_CHECK(hipMemcpyAsync(d->aos, kl, sizeof(edgehip_keyline) * kn, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_kf_unpack, dim3((kn + kKfThreads - 1) / kKfThreads), dim3(kKfThreads), 0, c->stream, d->kl[seq], (int)kn, (const edgehip_keyline *)d->aos);
        EH_LAUNCH_CHECK();
    }
    EH_CHECK(hipMemcpyAsync(d->ks + seq, &k, sizeof k, hipMemcpyHostToDevice, c->stream));
    EH_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}
