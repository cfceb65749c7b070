// keyframe_constraint.hip — the metric use of the key-frame links: the reference's kfvo::OptimizeRelContraint (src/mtracklib/kfvo.cpp:527-604),
// its evaluation OptimizeRelConstraint1Iter (:344-420), the scale step optimizeScaleF2KF (:263-302) and the pruning pass
// mutualExclusionSimple (:423-522), for every sequence's current key frame (keyframe_track.hip) against a ring slot, for whole batches.
//
// Two launches per constraint call, on the context's stream:
//   gather   one thread per walked KeyLine resolves its link ONCE and writes a compact row: the unprojected point (3 doubles), rho, s_rho
//            and p_m of the walked KeyLine, p_m, u_m, rho, s_rho of its partner, a valid flag, and a zero residual: 92 B per KeyLine
//            (8 doubles, 3 float2, one int32).
//            The iter_max + 2 evaluations then stream coalesced rows instead of chasing the links each time.
//   solve    ONE workgroup per sequence runs the whole Levenberg-Marquardt schedule inside one launch.  An evaluation: thread t takes the
//            rows t, t + 512, ... in that order and keeps 21 (JtJ, upper triangle) + 6 (JtF) + 1 (E) fp64 sums and two counts; the sums
//            go through the wave tree of wave_reduce.h, then the 8 waves are added in index order through LDS.  The order is fixed by the
//            row index alone: no float atomics, and the result does not depend on arrival order, the batch size or the sequence's index.
//            Thread 0 does the 6x6 solve (la::Cholesky<6>: TooN's L D L^T), SO3::exp, coerce and the gain rule, and hands the candidate
//            pose to the others through LDS.  The residual row lives in the scratch, one double per KeyLine, written and re-read by the
//            thread that owns the row.  The same launch makes ln(BRelRot), the inverse and optimizeScaleF2KF's two sums.
//   mutex    mutualExclusionSimple, one thread per KeyLine: the loop writes only the link of the KeyLine it is on, and reads the other
//            list's links and the p_m / u_m of its own list, so it is order-free.
//
// The rules, in the reference's types (tests/keyframe_constraint_port.py restates them; TooN's products are row dot products, 0 += in
// index order):
//   per linked KeyLine    Rx0 = BRelRot * unprojectHomCordVec(p_m.x, p_m.y, rho) (cam_model.h:163-169); q1 = projectHomCordVec(Rx0 + BRelPos)
//            (:146-152); f = (q1 - p_b) . u_b; dfdx = (q1.z*zfm*u_b.x, q1.z*zfm*u_b.y, -q1.z*q1.x*u_b.x - q1.z*q1.y*u_b.y); E += f*f;
//            stddev = sqrt(1 + ((dfdx . BRelPos) * s_rho / q1.z)^2); weight = k_huber / |residual| when k_huber > 0 && |residual| > k_huber,
//            else 1 and an inlier; residual = f AFTER the weight was read; row = weight * [dfdx, dfdx * crossMatrix(Rx0).T()] / stddev,
//            value f * (weight / stddev).  p_m, u_m are the records' floats, rho and s_rho their doubles, everything else fp64.
//   residual is one array for the whole call: every evaluation overwrites it, rejected steps included (no swap as in Minimizer_RV_KF).
//   schedule   two evaluations at the start pose (the first with all weights 1, its E thrown away); u = 1e-3 * max_element(JtJ), v = 2;
//            then iter_max steps: dX = Cholesky<6>(JtJ + u I).backsub(-JtF); BRelPosNew = BRelPos + dX[0:3]; BRelRotNew =
//            coerce(exp(dX[3:6]) * BRelRot); gain = (E - Enew) / (0.5 dX . (u dX - JtF)); gain > 0 accepts, u *= max(0.33, 1 - (2 gain - 1)^3),
//            v = 2; else u *= v, v *= 2.
//   optimizeScaleF2KF     at the final pose, with kfvo::unProject / kfvo::project (kfvo.h:42-48: the vector times ONE reciprocal, not the
//            camera's divisions): q = 1 / (BRelRot * x + BRelPos).z; for q > 0: v = s_rho^2 (q / rho)^2 + s_rho_b^2, rTr0 += q^2 / v,
//            rTr += rho_b^2 / v; Kp = rTr / rTr0 when both are > 0, else 1; W_Kp = rTr0.
// Where the reference has no defined result (it aborts in SO3::coerce's assertion, or reads out of bounds) the device has its own rule,
// edgehip.h: guard bits 0, 1, 2.
#include "keyframe_track.h"
#include "wave_reduce.h"

#include "rebvo/linalg.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace la = rebvo::la;

namespace edgehip {

constexpr int kKcGatherThreads = 256;
constexpr int kKcThreads = 512;
constexpr int kKcWaves = kKcThreads / 64;

struct KcRows {              // [nseq][cap] each
    double *x0, *x1, *x2;    // unprojectHomCordVec of the walked KeyLine
    double *rho, *s_rho, *rho_b, *s_rho_b, *resid;
    float2 *p_m, *p_b, *u_b;
    int32_t *valid;
};

struct KcArgs {
    KcRows r;
    const KlSoA *kf_kl, *slot_kl;
    const int32_t *slot_kn;
    const KfSeq *ks;
    const SeqDev *seqs;
    const double *pose_in;   // [nseq][13]: Pose, Pos, K; null: seq_state's
    edgehip_kf_constraint *out;
    int nseq, cap, direction, iter_max;
    double k_huber, zfm;
};

// KeyLines of the walked list and of the list its links index; a sequence without a key frame walks nothing
__device__ __forceinline__ void kc_counts(const KfSeq &k, int slot_kn, int cap, int direction, int &n, int &nb) {
    const int kf = k.kf_count > 0 ? max(0, min(k.kn, cap)) : 0, sl = k.kf_count > 0 ? max(0, min(slot_kn, cap)) : 0;
    n = direction ? sl : kf;
    nb = direction ? kf : sl;
}

__global__ __launch_bounds__(kKcGatherThreads) void k_kc_gather(KcArgs a) {
    const int seq = blockIdx.y, i = blockIdx.x * kKcGatherThreads + threadIdx.x;
    int n, nb;
    kc_counts(a.ks[seq], a.slot_kn[seq], a.cap, a.direction, n, nb);
    if (i >= n) return;
    const KlSoA &own = a.direction ? a.slot_kl[seq] : a.kf_kl[seq], &oth = a.direction ? a.kf_kl[seq] : a.slot_kl[seq];
    const int link = a.direction ? own.m_id_kf[i] : own.m_id_f[i];
    const size_t o = (size_t)seq * a.cap + i;
    a.r.resid[o] = 0.0;      // residual = Zeros (kfvo.cpp:548-549)
    if (link < 0 || link >= nb) {
        a.r.valid[o] = 0;
        if (link >= nb) atomicOr(&a.out[seq].guard, 4);
        return;
    }
    const float2 pm = own.p_m[i];
    const double rho = own.rho[i];
    a.r.x0[o] = (double)pm.x / rho / a.zfm;
    a.r.x1[o] = (double)pm.y / rho / a.zfm;
    a.r.x2[o] = 1.0 / rho;
    a.r.rho[o] = rho; a.r.s_rho[o] = own.s_rho[i]; a.r.p_m[o] = pm;
    a.r.p_b[o] = oth.p_m[link]; a.r.u_b[o] = oth.u_m[link];
    a.r.rho_b[o] = oth.rho[link]; a.r.s_rho_b[o] = oth.s_rho[link];
    a.r.valid[o] = 1;
}

struct KcShared {
    double part[kKcWaves][kNumSums];
    double sum[kNumSums];
    double R[9], T[3];       // the pose the next pass evaluates
    int cnt[2];
    int go;
    // thread 0's state between the passes (in LDS, not in registers every lane would have to set aside)
    double Ra[9], Ta[3];     // the last accepted pose
    double JtJ[36], JtF[6], dX[6];
    double E, E0, u, v;
    int links, inliers, evals, accepted, guard;
};

// One pass of the workgroup over the sequence's rows at the pose in sh.R / sh.T.  scale == 0: OptimizeRelConstraint1Iter — sh.sum =
// 21 JtJ (upper triangle, row by row), 6 JtF, E; sh.cnt = match_num.  scale == 1: optimizeScaleF2KF — sh.sum[0] = rTr0, sh.sum[1] = rTr.
// Ends behind a __syncthreads(): every thread may read sh.sum / sh.cnt.
__device__ __forceinline__ void kc_pass(const KcArgs &a, KcShared &sh, const size_t base, const int n, const int scale) {
    double R[9], T[3];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = sh.R[k];
#pragma unroll
    for (int k = 0; k < 3; k++) T[k] = sh.T[k];
    double sums[kNumSums];
#pragma unroll
    for (int k = 0; k < kNumSums; k++) sums[k] = 0.0;
    int c0 = 0, c1 = 0;
    for (int i = threadIdx.x; i < n; i += kKcThreads) {
        const size_t o = base + i;
        if (!a.r.valid[o]) continue;
        if (scale) {
            const float2 pm = a.r.p_m[o];
            const double rho = a.r.rho[o], s_rho = a.r.s_rho[o], rho_b = a.r.rho_b[o], s_rho_b = a.r.s_rho_b[o];
            const double iz = 1 / rho;
            const double x[3] = {(double)pm.x / a.zfm * iz, (double)pm.y / a.zfm * iz, 1.0 * iz};
            double s = 0;
            s += R[6] * x[0]; s += R[7] * x[1]; s += R[8] * x[2];
            const double q = 1.0 * (1 / (s + T[2]));
            if (q > 0) {
                const double v = s_rho * s_rho * (q / rho) * (q / rho) + s_rho_b * s_rho_b;
                sums[0] += q * q / v;
                sums[1] += rho_b * rho_b / v;
            }
            continue;
        }
        const double x[3] = {a.r.x0[o], a.r.x1[o], a.r.x2[o]};
        const float2 pb = a.r.p_b[o], ub = a.r.u_b[o];
        const double s_rho = a.r.s_rho[o];
        double Rx[3], p[3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            double s = 0;
            s += R[3 * r] * x[0]; s += R[3 * r + 1] * x[1]; s += R[3 * r + 2] * x[2];
            Rx[r] = s;
            p[r] = s + T[r];
        }
        const double q0 = p[0] / p[2] * a.zfm, q1 = p[1] / p[2] * a.zfm, q2 = 1 / p[2];
        const double ux = (double)ub.x, uy = (double)ub.y;
        double f = (q0 - (double)pb.x) * ux + (q1 - (double)pb.y) * uy;
        const double d[3] = {q2 * a.zfm * ux, q2 * a.zfm * uy, -q2 * q0 * ux - q2 * q1 * uy};
        sums[27] += f * f;
        double dt = 0;
        dt += d[0] * T[0]; dt += d[1] * T[1]; dt += d[2] * T[2];
        const double sd = dt * s_rho / q2;
        const double stddev = sqrt(1.0 * 1.0 + sd * sd);
        const double res = a.r.resid[o];
        double weight = 1;
        c0++;
        if (a.k_huber > 0 && fabs(res) > a.k_huber) weight = a.k_huber / fabs(res);
        else c1++;
        a.r.resid[o] = f;
        f *= weight / stddev;
        const double wd[3] = {weight * d[0], weight * d[1], weight * d[2]};
        // crossMatrix(Rx0).T() (toon_util.h:93-97), the product's zero terms included
        const double C[9] = {0, Rx[2], -Rx[1], -Rx[2], 0, Rx[0], Rx[1], -Rx[0], 0};
        double J[6];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            J[c] = wd[c] / stddev;
            double s = 0;
            s += wd[0] * C[c]; s += wd[1] * C[3 + c]; s += wd[2] * C[6 + c];
            J[3 + c] = s / stddev;
        }
        int k = 0;
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
            for (int c = r; c < 6; c++) sums[k++] += J[r] * J[c];
#pragma unroll
        for (int r = 0; r < 6; r++) sums[21 + r] += J[r] * f;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int idx = wave_reduce28(sums, lane);
    if (idx < kNumSums && !(lane & 1)) sh.part[wave][idx] = sums[0];
#pragma unroll
    for (int off = 32; off; off >>= 1) { c0 += __shfl_xor(c0, off, 64); c1 += __shfl_xor(c1, off, 64); }
    if (lane == 0) { atomicAdd(&sh.cnt[0], c0); atomicAdd(&sh.cnt[1], c1); }
    __syncthreads();
    if (threadIdx.x < kNumSums) {
        double s = 0;
        for (int w = 0; w < kKcWaves; w++) s += sh.part[w][threadIdx.x];
        sh.sum[threadIdx.x] = s;
    }
    __syncthreads();
}

__device__ inline bool kc_finite(const la::Mat<6, 6> &A) {
    bool ok = true;
    for (int i = 0; i < 36; i++) ok = ok && isfinite(A.a[i]);
    return ok;
}

// ---- thread 0 between the passes (not inlined: their registers are one lane's, and the passes' loop keeps its own) --------------------
// the start pose (kfvo.cpp:538-544) -> sh.R / sh.T, and the state cleared
__device__ __noinline__ void kc_lead_start(const KcArgs &a, KcShared &sh, const int seq) {
    const KfSeq &k = a.ks[seq];
    la::Mat<3, 3> Pose, KP, R;
    la::Vec<3> Pos, KPos, T;
    double K;
    if (a.pose_in) {
        const double *pi = a.pose_in + (size_t)seq * 13;
        for (int i = 0; i < 9; i++) Pose.a[i] = pi[i];
        for (int i = 0; i < 3; i++) Pos[i] = pi[9 + i];
        K = pi[12];
    } else {   // localPose = Pose * R, localPos = Pos - localPose * V * K (rebvo_second_t.cpp:435-436), as k_kf_setup takes them
        const edgehip_seq_state &p = a.seqs[seq].pub;
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) Pose(r, c) = p.Pose[r * 3 + 0] * p.R[0 * 3 + c] + p.Pose[r * 3 + 1] * p.R[1 * 3 + c] + p.Pose[r * 3 + 2] * p.R[2 * 3 + c];
        for (int i = 0; i < 3; i++) Pos[i] = p.Pos[i] - (Pose(i, 0) * p.V[0] + Pose(i, 1) * p.V[1] + Pose(i, 2) * p.V[2]) * p.K;
        K = p.K;
    }
    for (int i = 0; i < 9; i++) KP.a[i] = k.pose.Pose[i];
    for (int i = 0; i < 3; i++) KPos[i] = k.pose.Pos[i];
    if (a.direction) {   // :538-541
        R = la::transpose(KP) * Pose;
        T = (la::transpose(KP) * (Pos - KPos)) / K;
    } else {             // :542-544
        R = la::transpose(Pose) * KP;
        T = (la::transpose(Pose) * (KPos - Pos)) / k.pose.K;
    }
    for (int i = 0; i < 9; i++) sh.R[i] = sh.Ra[i] = R.a[i];
    for (int i = 0; i < 3; i++) sh.T[i] = sh.Ta[i] = T[i];
    for (int i = 0; i < 36; i++) sh.JtJ[i] = 0;
    for (int i = 0; i < 6; i++) sh.JtF[i] = sh.dX[i] = 0;
    sh.E = sh.E0 = sh.u = 0; sh.v = 2;
    sh.links = sh.inliers = sh.evals = sh.accepted = sh.guard = 0;
    sh.cnt[0] = sh.cnt[1] = 0;
    sh.go = 1;
}

// behind evaluation `ev`: the schedule of kfvo.cpp:552-589, and the next candidate pose -> sh.R / sh.T (or sh.go = 0)
__device__ __noinline__ void kc_lead_step(KcShared &sh, const int ev, const int n_eval) {
    sh.links = sh.cnt[0]; sh.inliers = sh.cnt[1];
    sh.cnt[0] = sh.cnt[1] = 0;
    sh.evals++;
    la::Mat<6, 6> JtJ;
    la::Vec<6> JtF, dX = la::Vec<6>::zeros();
    double u = sh.u, v = sh.v;
    if (ev <= 1) {            // the first evaluation's E is thrown away; E0, JtJ, JtF are the second's
        int k = 0;
        for (int r = 0; r < 6; r++)
            for (int c = r; c < 6; c++) { JtJ(r, c) = sh.sum[k]; JtJ(c, r) = sh.sum[k]; k++; }
        for (int r = 0; r < 6; r++) JtF[r] = sh.sum[21 + r];
        sh.E = sh.E0 = sh.sum[27];
        double m = JtJ.a[0];   // TooN::max_element(JtJ).first
        for (int i = 1; i < 36; i++) if (JtJ.a[i] > m) m = JtJ.a[i];
        u = 1e-3 * m; v = 2;
    } else {
        for (int i = 0; i < 36; i++) JtJ.a[i] = sh.JtJ[i];
        for (int i = 0; i < 6; i++) { JtF[i] = sh.JtF[i]; dX[i] = sh.dX[i]; }
        const double En = sh.sum[27];
        const la::Vec<6> h = 0.5 * dX;
        const double gain = (sh.E - En) / la::dot(h, u * dX - JtF);
        if (gain > 0) {
            sh.E = En;
            for (int i = 0; i < 9; i++) sh.Ra[i] = sh.R[i];
            for (int i = 0; i < 3; i++) sh.Ta[i] = sh.T[i];
            int k = 0;
            for (int r = 0; r < 6; r++)
                for (int c = r; c < 6; c++) { JtJ(r, c) = sh.sum[k]; JtJ(c, r) = sh.sum[k]; k++; }
            for (int r = 0; r < 6; r++) JtF[r] = sh.sum[21 + r];
            const double g = 2 * gain - 1;
            u *= fmax(0.33, 1 - (g * g * g));
            v = 2;
            sh.accepted++;
        } else {
            u *= v;
            v *= 2;
        }
    }
    if (ev >= 1 && ev + 1 < n_eval) {   // the next step's candidate
        bool ok = kc_finite(JtJ);
        if (ok) {
            dX = la::Cholesky<6>(JtJ + la::Mat<6, 6>::identity(u)).backsub(-JtF);
            for (int i = 0; i < 6; i++) ok = ok && isfinite(dX[i]);
        }
        if (ok) {
            la::Mat<3, 3> R;
            for (int i = 0; i < 9; i++) R.a[i] = sh.Ra[i];
            const la::Mat<3, 3> Rn = la::so3_coerce(la::so3_exp(la::slice<3>(dX, 3)) * R);
            for (int i = 0; i < 9; i++) sh.R[i] = Rn.a[i];
            for (int i = 0; i < 3; i++) sh.T[i] = sh.Ta[i] + dX[i];
        } else {
            sh.guard |= 1;
            sh.go = 0;
        }
    }
    for (int i = 0; i < 36; i++) sh.JtJ[i] = JtJ.a[i];
    for (int i = 0; i < 6; i++) { sh.JtF[i] = JtF[i]; sh.dX[i] = dX[i]; }
    sh.u = u; sh.v = v;
}

__device__ __noinline__ void kc_lead_finish(const KcArgs &a, KcShared &sh, const int seq) {
    edgehip_kf_constraint &o = a.out[seq];
    la::Mat<3, 3> R;
    la::Mat<6, 6> JtJ;
    for (int i = 0; i < 9; i++) R.a[i] = sh.Ra[i];
    for (int i = 0; i < 36; i++) JtJ.a[i] = sh.JtJ[i];
    const la::Vec<3> w = la::so3_ln(R);
    for (int i = 0; i < 3; i++) { o.X[i] = sh.Ta[i]; o.X[3 + i] = w[i]; }
    const la::Mat<6, 6> Inv = la::Cholesky<6>(JtJ).inverse();
    for (int i = 0; i < 36; i++) { o.W_X[i] = JtJ.a[i]; o.R_X[i] = Inv.a[i]; }
    o.ratio = sh.E / sh.E0; o.E = sh.E; o.E0 = sh.E0;
    if (a.direction) {
        const double rTr0 = sh.sum[0], rTr = sh.sum[1];
        o.Kp = (rTr0 > 0 && rTr > 0) ? (rTr / rTr0) : 1;
        o.W_Kp = rTr0;
    } else {
        o.Kp = 0; o.W_Kp = 0;
    }
    int guard = sh.guard;
    if (sh.links < 6) guard |= 2;
    o.links = sh.links; o.inliers = sh.inliers; o.evals = sh.evals; o.accepted = sh.accepted;
    o.guard |= guard;   // (bit 2 is the gather's)
    o.pad = 0;
}

__global__ __launch_bounds__(kKcThreads) void k_kc_solve(KcArgs a) {
    __shared__ KcShared sh;
    const int seq = blockIdx.x;
    const size_t base = (size_t)seq * a.cap;
    int n, nb;
    kc_counts(a.ks[seq], a.slot_kn[seq], a.cap, a.direction, n, nb);
    const bool lead = threadIdx.x == 0;
    if (lead) kc_lead_start(a, sh, seq);
    __syncthreads();
    const int n_eval = a.iter_max + 2;
    for (int ev = 0; ev < n_eval; ev++) {
        kc_pass(a, sh, base, n, 0);
        if (lead) kc_lead_step(sh, ev, n_eval);
        __syncthreads();
        if (!sh.go) break;
    }
    if (a.direction) {   // optimizeScaleF2KF at the final pose
        if (lead) {
            for (int i = 0; i < 9; i++) sh.R[i] = sh.Ra[i];
            for (int i = 0; i < 3; i++) sh.T[i] = sh.Ta[i];
        }
        __syncthreads();
        kc_pass(a, sh, base, n, 1);
    }
    if (lead) kc_lead_finish(a, sh, seq);
}

struct KcMutexArgs {
    const KlSoA *kf_kl, *slot_kl;
    const int32_t *slot_kn;
    const KfSeq *ks;
    int32_t *counts;         // [nseq][2], zeroed
    int cap, kf_to_frame, discard;
    double dist_t;
};

__global__ __launch_bounds__(kKcGatherThreads) void k_kc_mutex(KcMutexArgs a) {
    const int seq = blockIdx.y, i = blockIdx.x * kKcGatherThreads + threadIdx.x, lane = threadIdx.x & 63;
    int n, nb;
    kc_counts(a.ks[seq], a.slot_kn[seq], a.cap, !a.kf_to_frame, n, nb);
    bool seen = false, kept = false;
    if (i < n) {
        const KlSoA &own = a.kf_to_frame ? a.kf_kl[seq] : a.slot_kl[seq], &oth = a.kf_to_frame ? a.slot_kl[seq] : a.kf_kl[seq];
        int32_t *own_link = a.kf_to_frame ? own.m_id_f : own.m_id_kf;
        const int32_t *oth_link = a.kf_to_frame ? oth.m_id_kf : oth.m_id_f;
        const int m_f = own_link[i];
        if (m_f >= 0 && m_f < nb) {
            seen = true;
            const int m_b = oth_link[m_f];
            if (m_b < 0) {
                if (a.discard) own_link[i] = -1;
            } else if (m_b < n) {
                const float2 p = own.p_m[i], q = own.p_m[m_b];
                const float dx = p.x - q.x, dy = p.y - q.y;
                double dist;
                if (a.kf_to_frame) dist = (double)(float)sqrt((double)(dx * dx + dy * dy));   // util::norm<float>: sqrt of the float sum, the float overload
                else { const float2 um = own.u_m[i]; dist = (double)fabsf(dx * um.x + dy * um.y); }
                if (dist > a.dist_t) own_link[i] = -1;
                else kept = true;
            }
        }
    }
    const int c0 = __popcll(__ballot(seen)), c1 = __popcll(__ballot(kept));
    if (lane == 0) {
        if (c0) atomicAdd(&a.counts[2 * seq], c0);
        if (c1) atomicAdd(&a.counts[2 * seq + 1], c1);
    }
}

}  // namespace edgehip

using namespace edgehip;

namespace {
struct KcLayout {
    size_t x0, x1, x2, rho, s_rho, rho_b, s_rho_b, resid, p_m, p_b, u_b, valid, pose, out, total;
};
KcLayout kc_layout(size_t B, size_t cap) {
    KcLayout y;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; };
    const size_t kl = B * cap;
    y.x0 = take(kl * 8); y.x1 = take(kl * 8); y.x2 = take(kl * 8);
    y.rho = take(kl * 8); y.s_rho = take(kl * 8); y.rho_b = take(kl * 8); y.s_rho_b = take(kl * 8); y.resid = take(kl * 8);
    y.p_m = take(kl * 8); y.p_b = take(kl * 8); y.u_b = take(kl * 8);
    y.valid = take(kl * 4);
    y.pose = take(B * 13 * 8);
    y.out = take(B * sizeof(edgehip_kf_constraint));
    y.total = at;
    return y;
}

int kc_scratch(edgehip_ctx *c, const char *who, const KcLayout &y) {
    auto *d = c->kftrack;
    if (d->kc_arena) return 0;
    void *p = nullptr;
    if (hipMalloc(&p, y.total) != hipSuccess) {
        (void)hipGetLastError();
        set_error(std::string(who) + ": scratch allocation failed (92 B x max_points x nseq)");
        return EDGEHIP_ERR_MEMORY;
    }
    d->kc_arena = p;
    return 0;
}
}  // namespace

void edgehip::kf_constraint_free(edgehip_ctx *c) {
    auto *d = c->kftrack;
    if (!d || !d->kc_arena) return;
    (void)hipFree(d->kc_arena);
    d->kc_arena = nullptr;
    d->kc_ms[0] = d->kc_ms[1] = 0;
}

// behind kf_entry: whatever this returns, the caller then says it is done with the slot
static int kc_constraint_run(edgehip_ctx *c, const char *who, int slot_new, const double *Pose, const double *Pos, const double *K,
                             const edgehip_kf_constraint_args *args, edgehip_kf_constraint *out) {
    const bool given = Pose != nullptr;
    auto *d = c->kftrack;
    const size_t B = c->plan.nseq, cap = c->plan.cap;
    const KcLayout y = kc_layout(B, cap);
    if (int e = kc_scratch(c, who, y)) return e;
    uint8_t *base = (uint8_t *)d->kc_arena;
    KcArgs a;
    a.r.x0 = (double *)(base + y.x0); a.r.x1 = (double *)(base + y.x1); a.r.x2 = (double *)(base + y.x2);
    a.r.rho = (double *)(base + y.rho); a.r.s_rho = (double *)(base + y.s_rho);
    a.r.rho_b = (double *)(base + y.rho_b); a.r.s_rho_b = (double *)(base + y.s_rho_b); a.r.resid = (double *)(base + y.resid);
    a.r.p_m = (float2 *)(base + y.p_m); a.r.p_b = (float2 *)(base + y.p_b); a.r.u_b = (float2 *)(base + y.u_b);
    a.r.valid = (int32_t *)(base + y.valid);
    a.kf_kl = d->kl_dev; a.slot_kl = kldev(c, slot_new);
    a.slot_kn = c->kn_slot + (size_t)slot_new * B;
    a.ks = d->ks; a.seqs = c->seq;
    a.pose_in = nullptr;
    a.out = (edgehip_kf_constraint *)(base + y.out);
    a.nseq = (int)B; a.cap = (int)cap; a.direction = args->direction; a.iter_max = args->iter_max;
    a.k_huber = args->k_huber; a.zfm = c->plan.zfm;
    hipStream_t st = c->stream;
    std::vector<double> rows;
    if (given) {   // (pageable memory: the copy has left `rows` when the call returns; the call synchronises before that)
        rows.resize(B * 13);
        for (size_t s = 0; s < B; s++) {
            memcpy(&rows[s * 13], Pose + s * 9, 72);
            memcpy(&rows[s * 13 + 9], Pos + s * 3, 24);
            rows[s * 13 + 12] = K[s];
        }
        a.pose_in = (const double *)(base + y.pose);
    }
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    auto drop = [&]() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); };
    hipError_t err = given ? hipMemcpyAsync(base + y.pose, rows.data(), rows.size() * 8, hipMemcpyHostToDevice, st) : hipSuccess;
    if (err == hipSuccess) err = hipMemsetAsync(a.out, 0, sizeof(edgehip_kf_constraint) * B, st);
    for (int j = 0; j < 3 && err == hipSuccess; j++) err = hipEventCreate(&ev[j]);
    if (err == hipSuccess) err = hipEventRecord(ev[0], st);
    if (err == hipSuccess) {
        const unsigned tiles = (unsigned)((cap + kKcGatherThreads - 1) / kKcGatherThreads);
        hipLaunchKernelGGL(k_kc_gather, dim3(tiles, (unsigned)B), dim3(kKcGatherThreads), 0, st, a);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipEventRecord(ev[1], st);
    if (err == hipSuccess) {
        hipLaunchKernelGGL(k_kc_solve, dim3((unsigned)B), dim3(kKcThreads), 0, st, a);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipEventRecord(ev[2], st);
    if (err == hipSuccess) err = hipMemcpyAsync(out, a.out, sizeof(edgehip_kf_constraint) * B, hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    for (int j = 0; j < 2 && err == hipSuccess; j++) {
        float ms = 0;
        err = hipEventElapsedTime(&ms, ev[j], ev[j + 1]);
        d->kc_ms[j] = ms;
    }
    drop();
    EH_CHECK(err);
    return 0;
}

int edgehip_keyframe_constraint(edgehip_ctx *c, int slot_new, const double *Pose, const double *Pos, const double *K,
                                const edgehip_kf_constraint_args *args, edgehip_kf_constraint *out) {
    EH_ENTER(c);
    const char *who = "keyframe_constraint";
    if (!args || !out) { set_error("keyframe_constraint: null args or out"); return EDGEHIP_ERR_ARG; }
    if (args->iter_max < 0 || (args->direction != 0 && args->direction != 1)) {
        set_error("keyframe_constraint: iter_max must be >= 0 and direction 0 or 1");
        return EDGEHIP_ERR_ARG;
    }
    const int given = (Pose != nullptr) + (Pos != nullptr) + (K != nullptr);
    if (given != 0 && given != 3) { set_error("keyframe_constraint: Pose, Pos and K are given together (or all NULL)"); return EDGEHIP_ERR_ARG; }
    if (int e = kf_entry(c, slot_new, who)) return e;   // EDGEHIP_ERR_STATE, the slot's range, the slot's KeyLines turned
    const int e = kc_constraint_run(c, who, slot_new, Pose, Pos, K, args, out);
    const int r = slot_read_done(c, slot_new);          // on every path behind kf_entry, an error's included
    return e ? e : r;
}

int edgehip_keyframe_mutual_exclusion(edgehip_ctx *c, int slot_new, double dist_t, int discard_non_mutual, int kf_to_frame, int32_t *counts) {
    EH_ENTER(c);
    const char *who = "keyframe_mutual_exclusion";
    if (int e = kf_entry(c, slot_new, who)) return e;
    auto *d = c->kftrack;
    const size_t B = c->plan.nseq, cap = c->plan.cap;
    KcMutexArgs a;
    a.kf_kl = d->kl_dev; a.slot_kl = kldev(c, slot_new);
    a.slot_kn = c->kn_slot + (size_t)slot_new * B;
    a.ks = d->ks;
    a.counts = d->kc_counts;   // (its own 8 B per sequence, allocated with the key frames: pruning alone never allocates the rows)
    a.cap = (int)cap; a.kf_to_frame = kf_to_frame != 0; a.discard = discard_non_mutual != 0;
    a.dist_t = dist_t;
    EH_CHECK(hipMemsetAsync(a.counts, 0, B * 2 * 4, c->stream));
    const unsigned tiles = (unsigned)((cap + kKcGatherThreads - 1) / kKcGatherThreads);
    hipLaunchKernelGGL(k_kc_mutex, dim3(tiles, (unsigned)B), dim3(kKcGatherThreads), 0, c->stream, a);
    EH_LAUNCH_CHECK();
    if (int e = slot_read_done(c, slot_new)) return e;
    if (!counts) return 0;
    EH_CHECK(hipMemcpyAsync(counts, a.counts, B * 2 * 4, hipMemcpyDeviceToHost, c->stream));
    EH_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int edgehip_keyframe_constraint_ms(edgehip_ctx *c, double *gather_ms, double *solve_ms) {
    EH_ENTER(c);
    if (!c->kftrack) { set_error("keyframe_constraint_ms: key-frame tracking is not enabled"); return EDGEHIP_ERR_STATE; }
    if (gather_ms) *gather_ms = c->kftrack->kc_ms[0];
    if (solve_ms) *solve_ms = c->kftrack->kc_ms[1];
    return 0;
}
