// keyframe_reloc.hip — re-localise a frame against its sequence's key frames: the reference's kfvo::OptimizePosGT (src/mtracklib/kfvo.cpp:58-112)
// with kfvo::optimizeScale (:222-260), ring slot `slot` of every sequence against every selected key frame of the same sequence — the entries of
// its key-frame list (keyframe_list.hip) and its current key frame (keyframe_track.hip), the positions of keyframe_covis.hip — in one call.
// Read-only: the kernels below read the key-frame store, the list and the ring slot, and write only their own scratch.
//
// The minimisation is NOT restated here.  The selected (sequence, position) pairs of a pass are a batch of their own (KfBatch, ctx.h): every
// kernel of edgehip_minimizer_rv_kf — k_field_bin / k_field_raster, k_tvr_prepare, k_try_velrot_kf (tvr_body<true, true, false, true>),
// k_lm_step's LM_*_KF operations, k_count_forward — indexes its inputs by the `seq` it is given, so per-pair descriptor arrays make a pair look
// like a sequence, and stage_b.hip's own schedule (minimizer_kf_batch_enqueue) runs over them: ONE chain of 2 (iter_max + 1) dependent
// launches for all pairs of a pass, grid (tiles, 1, pairs).
//   a pair's query KlSoA      the slot's pointer set with m_id_f redirected to the pair's own link array
//   a pair's key-frame KlSoA  what the field and the evaluation read: rec (c_p, u_m, m_m, n_m), rho, s_rho
//
// Per call, on the context's stream:
//   k_rl_desc     the positions of every sequence (kf_position, keyframe_track.h: as the covisibility has them)
//   per pass of P = min(M, 8) positions:
//     k_rl_setup    per pair: selected or not, the two KlSoA, BRelRot / BRelPos / W0 (kfvo.cpp:62-68) as the minimiser's request
//     k_rl_gather   every selected key frame ONCE into the pair's rec / rho / s_rho: 48 B per KeyLine out of the 168-byte list records (read
//                   coalesced through LDS, k_kf_restore's way) or out of the current key frame's SoA
//     field + minimisation (stage_b.hip)
//     k_rl_finish   one workgroup per pair: optimizeScale's two sums, then (one lane) Kp, K, Pose, Pos (kfvo.cpp:89-96)
//
// optimizeScale's sums: lane l of the 256 adds its KeyLines l, l + 256, ... in that order, the 64 lanes of a wave are added by a butterfly,
// the 4 waves in wave order — a fixed order that depends on nothing but the pair's own KeyLines: the same bits alone, in any batch, under any
// to_mask.  No float atomics.
//
// Scratch (allocated on first use, freed with the key frames; NP = nseq x P pairs, T field tiles, nblk = ceil(max_points / 256)):
//   per pair and KeyLine   rec 32 B, rho 8, s_rho 8, residuals 3 x 8, bins 4 T
//   per pair               field16 plane, 256 B x nblk (carries, partial sums, block residuals), SeqDev, two KlSoA, request, result, bin counts
//   per (sequence, position)   links max_points x 4 B, result 488 B, descriptor
#include "keyframe_track.h"
#include "rebvo/linalg.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace edgehip {
namespace la = rebvo::la;

constexpr int kRlThreads = 256;
constexpr int kRlMaxPass = 8;        // positions served at a time (keyframe_covis.hip's kCvMaxPlanes)
constexpr int kRlBinTiles = 256;     // stage_b.hip's kMaxTiles: bin counters per list
constexpr int kRlFieldTile = 64;     // stage_b.hip's FT
constexpr int kRlKlBytes = (int)sizeof(edgehip_keyline);
static_assert(kRlKlBytes == 168 && (kRlThreads * kRlKlBytes) % 16 == 0, "a tile of list records is a whole number of 16-byte words");
static_assert(sizeof(edgehip_kf_reloc) == 488 && sizeof(edgehip_kf_reloc_args) == 32, "include/edgehip.h");

struct RlArgs {
    CvKf *desc;                      // [nseq][M + 1]
    KlSoA *kl_cur, *kl_kf;           // [NP]
    int32_t *kn_cur, *kn_kf;         // [NP] 0 for a pair that is not served
    int32_t *pose_guard;             // [NP]
    MatchRec *rec;                   // [NP][cap]
    double *rho, *s_rho;             // [NP][cap]
    int32_t *links;                  // [nseq][M][cap]
    int32_t *link_kn;                // [nseq][M] the query's KeyLines, -1: not served
    edgehip_kf_request *req;         // [NP]
    edgehip_kf_result *res;          // [NP]
    SeqDev *seq;                     // [NP]
    edgehip_kf_reloc *out;           // [nseq][M]
    const uint8_t *mask;             // [nseq][M], or null
    const double *s_rho_q;           // [nseq]
    int nseq, M, P, cap;
    double zfm;
};

__global__ void k_rl_desc(RlArgs a, const KfSeq *__restrict__ ks, KfListDev l, const int32_t *__restrict__ slot_kn,
                          const edgehip_kf_pose *__restrict__ pose_in, const SeqDev *__restrict__ seqs, const edgehip_nav *__restrict__ nav) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.nseq * (a.M + 1)) return;
    a.desc[g] = kf_position(g / (a.M + 1), g % (a.M + 1), a.M, a.cap, ks, l, slot_kn, pose_in, seqs, nav);
}

// pair v = seq * P + pl of the pass that starts at position t0
__global__ void k_rl_setup(RlArgs a, int t0, const KlSoA *__restrict__ slot_kl) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= a.nseq * a.P) return;
    const int seq = v / a.P, t = t0 + v % a.P;
    const CvKf &q = a.desc[(size_t)seq * (a.M + 1) + a.M];
    const bool have = t < a.M;
    const CvKf &k = a.desc[(size_t)seq * (a.M + 1) + (have ? t : 0)];
    const bool on = have && k.kn >= 0 && q.kn >= 0 && (!a.mask || a.mask[(size_t)seq * a.M + t] != 0);
    a.kn_cur[v] = on ? q.kn : 0;
    a.kn_kf[v] = on ? k.kn : 0;
    KlSoA cur = slot_kl[seq];
    cur.m_id_f = have ? a.links + ((size_t)seq * a.M + t) * a.cap : nullptr;   // (a pair beyond M has no KeyLines: nothing is written through it)
    a.kl_cur[v] = cur;
    KlSoA kf;
    memset(&kf, 0, sizeof(kf));
    kf.rec = a.rec + (size_t)v * a.cap; kf.rho = a.rho + (size_t)v * a.cap; kf.s_rho = a.s_rho + (size_t)v * a.cap;
    a.kl_kf[v] = kf;
    edgehip_kf_request r;
    for (int i = 0; i < 6; i++) r.X0[i] = 0;
    r.Kr = 1; r.max_s_rho = 0;
    int bad = 0;
    if (on) {
        la::Mat<3, 3> Pt, Pq;
        la::Vec<3> d;
        for (int i = 0; i < 9; i++) { Pt.a[i] = k.Pose[i]; Pq.a[i] = q.Pose[i]; bad |= (k.Pose[i] != k.Pose[i]) | (q.Pose[i] != q.Pose[i]); }
        for (int i = 0; i < 3; i++) d[i] = q.Pos[i] - k.Pos[i];
        const la::Mat<3, 3> PtT = la::transpose(Pt);
        const la::Mat<3, 3> BRelRot = PtT * Pq;                  // kfvo.cpp:62
        const la::Vec<3> BRelPos = (PtT * d) / q.K;              // :63 — by the QUERY's K
        const la::Vec<3> W0 = la::so3_ln(BRelRot);               // :68 SO3<>(BRelRot).ln(): coerces first
        for (int i = 0; i < 3; i++) { r.X0[i] = BRelPos[i]; r.X0[3 + i] = W0[i]; }
        r.Kr = q.K / k.K;
        r.max_s_rho = a.s_rho_q[seq];
    }
    a.req[v] = r;
    a.pose_guard[v] = bad;
    if (have) {
        a.link_kn[(size_t)seq * a.M + t] = on ? q.kn : -1;
        if (!on) {
            edgehip_kf_reloc o;
            memset(&o, 0, sizeof(o));
            o.mnum = o.evals = o.accepted = o.guard = -1;
            a.out[(size_t)seq * a.M + t] = o;
        }
    }
}

// The selected key frames of a pass into the pairs' rec / rho / s_rho.  A list entry's tile of 256 records is 43 008 contiguous bytes: read as
// 16-byte words into LDS (coalesced), then each lane takes the 48 bytes it wants of its own record (168 B = 42 words apart: 2-way on the banks).
__global__ __launch_bounds__(kRlThreads) void k_rl_gather(RlArgs a, int t0, KfListDev l, const KlSoA *__restrict__ kf_kl) {
    typedef uint32_t u4v __attribute__((ext_vector_type(4)));
    __shared__ __align__(16) uint8_t img[kRlThreads * kRlKlBytes];
    const int seq = blockIdx.z, pl = blockIdx.y, tid = threadIdx.x, r0 = blockIdx.x * kRlThreads;
    const int v = seq * a.P + pl;
    const int kn = a.kn_kf[v];
    if (kn <= r0) return;                        // block-uniform: the pair is not served, or the list ends before this tile
    const CvKf &d = a.desc[(size_t)seq * (a.M + 1) + t0 + pl];   // (kn > 0: t0 + pl < M)
    const int i = r0 + tid;
    const size_t o = (size_t)v * a.cap + i;
    if (d.src >= 0) {
        // the words that hold the tile's records: the last one may reach 8 bytes past an odd list's end, still inside the entry (its stride is a
        // multiple of 16), and nothing reads those bytes out of the image
        const uint8_t *entry = l.rec + ((size_t)seq * l.capacity + d.src) * l.stride;
        const size_t b0 = (size_t)r0 * kRlKlBytes, b1 = (size_t)min(kn, r0 + kRlThreads) * kRlKlBytes;
        const int nw = (int)((b1 - b0 + 15) / 16);
        for (int t = tid; t < nw; t += kRlThreads)
            *reinterpret_cast<u4v *>(img + t * 16) = __builtin_nontemporal_load(reinterpret_cast<const u4v *>(entry + b0 + (size_t)t * 16));
        __syncthreads();
        if (i >= kn) return;
        const edgehip_keyline *r = reinterpret_cast<const edgehip_keyline *>(img + tid * kRlKlBytes);
        MatchRec m;
        m.c_px = r->c_p[0]; m.c_py = r->c_p[1]; m.u_mx = r->u_m[0]; m.u_my = r->u_m[1]; m.m_mx = r->m_m[0]; m.m_my = r->m_m[1]; m.n_m = r->n_m; m.pad = 0.f;
        a.rec[o] = m; a.rho[o] = r->rho; a.s_rho[o] = r->s_rho;
    } else {
        if (i >= kn) return;
        const KlSoA &s = kf_kl[seq];
        const float2 c_p = s.c_p[i], u_m = s.u_m[i], m_m = s.m_m[i];
        MatchRec m;
        m.c_px = c_p.x; m.c_py = c_p.y; m.u_mx = u_m.x; m.u_my = u_m.y; m.m_mx = m_m.x; m.m_my = m_m.y; m.n_m = s.n_m[i]; m.pad = 0.f;
        a.rec[o] = m; a.rho[o] = s.rho[i]; a.s_rho[o] = s.s_rho[i];
    }
}

// kfvo::optimizeScale (kfvo.cpp:222-260; unProject / project: kfvo.h:42-48) and OptimizePosGT's last lines (:89-96), one workgroup per pair
__global__ __launch_bounds__(kRlThreads) void k_rl_finish(RlArgs a, int t0) {
    __shared__ double s_R[9], s_p[3];
    __shared__ double s_sum[kRlThreads / 64][2];
    __shared__ int s_bad[kRlThreads / 64];
    const int v = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seq = v / a.P, t = t0 + v % a.P;
    if (t >= a.M || a.link_kn[(size_t)seq * a.M + t] < 0) return;   // block-uniform: k_rl_setup wrote the pair's -1 record
    const edgehip_kf_result &res = a.res[v];
    if (tid == 0) {
        const la::Mat<3, 3> R = la::so3_exp(la::Vec<3>{{res.X[3], res.X[4], res.X[5]}});   // :89 SO3<>(BRelRotW).get_matrix()
        for (int i = 0; i < 9; i++) s_R[i] = R.a[i];
        for (int i = 0; i < 3; i++) s_p[i] = res.X[i];
    }
    __syncthreads();
    const int kn = a.kn_cur[v], kn_kf = a.kn_kf[v];
    const KlSoA &kq = a.kl_cur[v];
    const double *rho_b = a.rho + (size_t)v * a.cap, *s_rho_b = a.s_rho + (size_t)v * a.cap;
    double rTr = 0, rTr0 = 0;
    int bad = 0;
    for (int i = tid; i < kn; i += kRlThreads) {
        const float2 p_m = kq.p_m[i];
        const double rho = kq.rho[i];
        // unProject: makeVector(q[0] / zfm, q[1] / zfm, 1) * (1 / q[2])
        const double ir = 1 / rho;
        const double ux = ((double)p_m.x / a.zfm) * ir, uy = ((double)p_m.y / a.zfm) * ir, uz = 1.0 * ir;
        double p[3];
        for (int r = 0; r < 3; r++) {
            double s = 0;
            s += s_R[3 * r] * ux; s += s_R[3 * r + 1] * uy; s += s_R[3 * r + 2] * uz;
            p[r] = s + s_p[r];
        }
        // project: makeVector(p[0] * zfm, p[1] * zfm, 1) * (1 / p[2])
        const double iz = 1 / p[2];
        const double q0 = (p[0] * a.zfm) * iz, q1 = (p[1] * a.zfm) * iz, q2 = 1.0 * iz;
        bad += !(isfinite(q0) && isfinite(q1) && isfinite(q2));
        const int id = kq.m_id_f[i];
        if (id >= 0 && id < kn_kf && q2 > 0) {
            const double s = kq.s_rho[i], sb = s_rho_b[id];
            const double vv = s * s * 1.0 * 1.0 + sb * sb;   // Kr = 1 inside (:226, :245)
            rTr0 += q2 * q2 / vv;
            rTr += q2 * rho_b[id] / vv;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        rTr0 += __shfl_xor(rTr0, o, 64);
        rTr += __shfl_xor(rTr, o, 64);
        bad += __shfl_xor(bad, o, 64);
    }
    if (lane == 0) { s_sum[wave][0] = rTr0; s_sum[wave][1] = rTr; s_bad[wave] = bad; }
    __syncthreads();
    if (tid != 0) return;
    rTr0 = s_sum[0][0]; rTr = s_sum[0][1]; bad = s_bad[0];
    for (int w = 1; w < kRlThreads / 64; w++) { rTr0 += s_sum[w][0]; rTr += s_sum[w][1]; bad += s_bad[w]; }
    const CvKf &k = a.desc[(size_t)seq * (a.M + 1) + t];
    edgehip_kf_reloc o;
    for (int i = 0; i < 6; i++) o.X[i] = res.X[i];
    for (int i = 0; i < 36; i++) o.RRV[i] = res.RRV[i];
    o.score_ratio = res.score_ratio; o.F = res.F; o.F0 = res.F0;
    o.Kp = (rTr0 > 0 && rTr > 0) ? (rTr0 / rTr) : 1;            // :255
    o.K = k.K * o.Kp;                                           // :93
    la::Mat<3, 3> Pt, R;
    for (int i = 0; i < 9; i++) { Pt.a[i] = k.Pose[i]; R.a[i] = s_R[i]; }
    const la::Mat<3, 3> Pc = la::so3_coerce(Pt);                // SO3<>(mkf.Pose)
    const la::Mat<3, 3> Po = Pc * R;                            // :95
    const la::Vec<3> pr = (Pc * la::Vec<3>{{s_p[0], s_p[1], s_p[2]}}) * o.K;   // :96, in that order
    for (int i = 0; i < 9; i++) o.Pose[i] = Po.a[i];
    for (int i = 0; i < 3; i++) o.Pos[i] = pr[i] + k.Pos[i];
    o.mnum = res.mnum; o.evals = res.evals; o.accepted = a.seq[v].eff_steps; o.guard = bad + a.pose_guard[v];
    a.out[(size_t)seq * a.M + t] = o;
}

}  // namespace edgehip

using namespace edgehip;

namespace {
struct RlLayout {
    size_t bins, resid, rec, rho, s_rho, field16, carry, partials, block_last, links, seq, kl_cur, kl_kf, req, res, bin_cnt, kn_cur, kn_kf, retuned,
        pose_guard, desc, out, link_kn, mask, pose, s_rho_q, total, zero_from;
};
RlLayout rl_layout(const edgehip_ctx *c, size_t M, size_t P) {
    RlLayout y;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; };
    const size_t B = c->plan.nseq, NP = B * P, cap = c->plan.cap, nblk = c->nblk_tvr;
    const size_t tiles = (size_t)((c->plan.w + kRlFieldTile - 1) / kRlFieldTile) * ((c->plan.h + kRlFieldTile - 1) / kRlFieldTile);
    y.bins = take(NP * tiles * cap * 4);
    y.resid = take(kResidBufs * NP * cap * 8);
    y.rec = take(NP * cap * sizeof(MatchRec)); y.rho = take(NP * cap * 8); y.s_rho = take(NP * cap * 8);
    y.field16 = take(NP * c->plan.f16stride * 2);
    y.carry = take(kResidBufs * NP * nblk * 8); y.partials = take(NP * nblk * kNumSums * 8); y.block_last = take(NP * nblk * 8);
    y.links = take(B * M * cap * 4);
    y.kl_cur = take(NP * sizeof(KlSoA)); y.kl_kf = take(NP * sizeof(KlSoA));
    y.req = take(NP * sizeof(edgehip_kf_request)); y.res = take(NP * sizeof(edgehip_kf_result));
    y.kn_cur = take(NP * 4); y.kn_kf = take(NP * 4); y.pose_guard = take(NP * 4);
    y.desc = take(B * (M + 1) * sizeof(CvKf)); y.out = take(B * M * sizeof(edgehip_kf_reloc)); y.link_kn = take(B * M * 4);
    y.mask = take(B * M); y.pose = take(B * sizeof(edgehip_kf_pose)); y.s_rho_q = take(B * 8);
    // cleared once, when the arena is allocated: the minimiser's state of a pair, the bin counters (the rasteriser leaves them at 0), build_field's
    // min_mod for a negative argument (0: every KeyLine, as edgehip_keyframe_list_restore leaves a restored slot's)
    y.zero_from = at;
    y.seq = take(NP * sizeof(SeqDev)); y.bin_cnt = take(NP * kRlBinTiles * 4); y.retuned = take(NP * 4);
    y.total = at;
    return y;
}
}  // namespace

void edgehip::kf_reloc_free(edgehip_ctx *c) {
    auto *d = c->kftrack;
    if (!d || !d->reloc_arena) return;
    (void)hipFree(d->reloc_arena);
    d->reloc_arena = nullptr; d->reloc_m = 0;
    d->reloc_ms[0] = d->reloc_ms[1] = 0;
}

extern "C" {

int edgehip_keyframe_relocalize(edgehip_ctx *c, int slot, const edgehip_kf_pose *pose, const double *s_rho_q, const uint8_t *to_mask,
                                const edgehip_kf_reloc_args *args, edgehip_kf_reloc *out, edgehip_kf_list_info *info) {
    EH_ENTER(c);
    const char *who = "keyframe_relocalize";
    auto *d = c->kftrack;
    if (!d) { set_error(std::string(who) + ": key-frame tracking is not enabled (edgehip_keyframe_track_enable)"); return EDGEHIP_ERR_STATE; }
    if (!args || !out || !s_rho_q) { set_error(std::string(who) + ": null args, s_rho_q or out"); return EDGEHIP_ERR_ARG; }
    if (args->field_radius < 1 || args->field_radius > 255) { set_error(std::string(who) + ": field_radius must be in [1, 255] (build_field's limit)"); return EDGEHIP_ERR_ARG; }
    if (args->iter_max < 0) { set_error(std::string(who) + ": iter_max < 0"); return EDGEHIP_ERR_ARG; }
    if (c->plan.cap > 65535) { set_error(std::string(who) + ": max_points above 65535 (16 bits of the field's KeyLine index)"); return EDGEHIP_ERR_ARG; }
    if (slot < 0 || slot >= c->plan.nslots) { set_error(std::string(who) + ": slot out of range"); return EDGEHIP_ERR_ARG; }
    if (((c->plan.w + kRlFieldTile - 1) / kRlFieldTile) * ((c->plan.h + kRlFieldTile - 1) / kRlFieldTile) > kRlBinTiles) {
        set_error(std::string(who) + ": the image has more field tiles than the binned build_field serves");
        return EDGEHIP_ERR_ARG;
    }
    const size_t B = c->plan.nseq, cap = c->plan.cap;
    const int M = d->list.hdr ? d->list.capacity + 1 : 1, P = std::min(M, kRlMaxPass);
    const size_t NP = B * P;
    const RlLayout y = rl_layout(c, M, P);
    hipStream_t st = c->stream;
    if (d->reloc_arena && d->reloc_m != M) {   // the list was enabled, freed or resized since
        EH_CHECK(hipStreamSynchronize(st));
        kf_reloc_free(c);
    }
    if (!d->reloc_arena) {
        void *p = nullptr;
        if (hipMalloc(&p, y.total) != hipSuccess) {
            (void)hipGetLastError();
            set_error(std::string(who) + ": scratch allocation failed (see include/edgehip.h for its size)");
            return EDGEHIP_ERR_MEMORY;
        }
        d->reloc_arena = p; d->reloc_m = M;
        EH_CHECK(hipMemsetAsync((uint8_t *)p + y.zero_from, 0, y.total - y.zero_from, st));
    }
    if (int e = rot_materialize_enqueue(c, slot)) return e;   // the slot's KeyLines as edgehip_download_keylines returns them
    if (int e = order_bc_after_a(c)) return e;
    uint8_t *base = (uint8_t *)d->reloc_arena;
    RlArgs a;
    a.desc = (CvKf *)(base + y.desc);
    a.kl_cur = (KlSoA *)(base + y.kl_cur); a.kl_kf = (KlSoA *)(base + y.kl_kf);
    a.kn_cur = (int32_t *)(base + y.kn_cur); a.kn_kf = (int32_t *)(base + y.kn_kf); a.pose_guard = (int32_t *)(base + y.pose_guard);
    a.rec = (MatchRec *)(base + y.rec); a.rho = (double *)(base + y.rho); a.s_rho = (double *)(base + y.s_rho);
    a.links = (int32_t *)(base + y.links); a.link_kn = (int32_t *)(base + y.link_kn);
    a.req = (edgehip_kf_request *)(base + y.req); a.res = (edgehip_kf_result *)(base + y.res);
    a.seq = (SeqDev *)(base + y.seq);
    a.out = (edgehip_kf_reloc *)(base + y.out);
    a.mask = nullptr; a.s_rho_q = (const double *)(base + y.s_rho_q);
    a.nseq = (int)B; a.M = M; a.P = P; a.cap = (int)cap; a.zfm = c->plan.zfm;
    // (pageable memory: the copies have left the caller's arrays when they return; the call synchronises anyway)
    EH_CHECK(hipMemcpyAsync(base + y.s_rho_q, s_rho_q, 8 * B, hipMemcpyHostToDevice, st));
    if (to_mask) {
        EH_CHECK(hipMemcpyAsync(base + y.mask, to_mask, B * M, hipMemcpyHostToDevice, st));
        a.mask = base + y.mask;
    }
    edgehip_kf_pose *pose_dev = nullptr;
    if (pose) {
        pose_dev = (edgehip_kf_pose *)(base + y.pose);
        EH_CHECK(hipMemcpyAsync(pose_dev, pose, sizeof(edgehip_kf_pose) * B, hipMemcpyHostToDevice, st));
    }
    KfBatch b = {};
    b.n = (int)NP;
    b.kl_kf = a.kl_kf; b.kl_cur = a.kl_cur; b.kn_kf = a.kn_kf; b.kn_cur = a.kn_cur;
    b.retuned = (const float *)(base + y.retuned);
    b.bin_cnt = (int32_t *)(base + y.bin_cnt); b.bins = (int32_t *)(base + y.bins);
    b.field16 = (uint16_t *)(base + y.field16); b.field_radius = args->field_radius;
    b.seq = a.seq;
    b.resid = (double *)(base + y.resid); b.resid_carry = (double *)(base + y.carry);
    b.partials = (double *)(base + y.partials); b.block_last = (double *)(base + y.block_last);
    b.framecount = nullptr;
    b.req = a.req; b.res = a.res;
    b.f32 = 0;

    std::vector<hipEvent_t> ev;
    auto mark = [&]() -> hipError_t {
        hipEvent_t e = nullptr;
        hipError_t r = hipEventCreate(&e);
        if (r != hipSuccess) return r;
        ev.push_back(e);
        return hipEventRecord(e, st);
    };
    auto drop = [&]() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); ev.clear(); };
    const unsigned tiles = (unsigned)((cap + kRlThreads - 1) / kRlThreads);
    hipError_t err = mark();
    int rc = 0;
    if (err == hipSuccess) {
        hipLaunchKernelGGL(k_rl_desc, dim3((unsigned)((B * (M + 1) + 63) / 64)), dim3(64), 0, st, a, (const KfSeq *)d->ks, d->list,
                           (const int32_t *)(c->kn_slot + (size_t)slot * B), (const edgehip_kf_pose *)pose_dev, (const SeqDev *)c->seq,
                           (const edgehip_nav *)c->nav_dev);
        err = hipGetLastError();
    }
    // events: 0 | prepare | 1 | solve | 2 (| prepare | 3 | solve | 4 ...)
    for (int t0 = 0; t0 < M && err == hipSuccess && rc == 0; t0 += P) {
        hipLaunchKernelGGL(k_rl_setup, dim3((unsigned)((NP + 63) / 64)), dim3(64), 0, st, a, t0, (const KlSoA *)kldev(c, slot));
        if ((err = hipGetLastError()) != hipSuccess) break;
        hipLaunchKernelGGL(k_rl_gather, dim3(tiles, P, (unsigned)B), dim3(kRlThreads), 0, st, a, t0, d->list, (const KlSoA *)d->kl_dev);
        if ((err = hipGetLastError()) != hipSuccess) break;
        if ((rc = build_field_batch_enqueue(c, b, args->field_radius, args->field_min_mod)) != 0) break;
        if ((err = mark()) != hipSuccess) break;
        if ((rc = minimizer_kf_batch_enqueue(c, b, 5.0, 30.0 * M_PI / 180.0, args->rho_tol, args->iter_max, args->rew_dis, 0)) != 0) break;
        hipLaunchKernelGGL(k_rl_finish, dim3((unsigned)NP), dim3(kRlThreads), 0, st, a, t0);
        if ((err = hipGetLastError()) != hipSuccess) break;
        err = mark();
    }
    if (err != hipSuccess || rc != 0) {
        (void)hipStreamSynchronize(st);
        drop();
        (void)slot_read_done(c, slot);
        if (rc != 0) return rc;
        EH_CHECK(err);
    }
    std::vector<KfListSeq> ls(B);
    std::vector<KfSeq> ks(info ? B : 0);
    err = hipMemcpyAsync(out, a.out, sizeof(edgehip_kf_reloc) * B * M, hipMemcpyDeviceToHost, st);
    if (err == hipSuccess && info) {
        if (d->list.hdr) err = hipMemcpyAsync(ls.data(), d->list.ls, sizeof(KfListSeq) * B, hipMemcpyDeviceToHost, st);
        if (err == hipSuccess) err = hipMemcpyAsync(ks.data(), d->ks, sizeof(KfSeq) * B, hipMemcpyDeviceToHost, st);
    }
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    if (err == hipSuccess) {
        d->reloc_ms[0] = d->reloc_ms[1] = 0;
        for (size_t j = 0; j + 1 < ev.size() && err == hipSuccess; j++) {
            float ms = 0;
            err = hipEventElapsedTime(&ms, ev[j], ev[j + 1]);
            d->reloc_ms[j & 1] += ms;
        }
    }
    drop();
    if (err != hipSuccess) (void)slot_read_done(c, slot);
    EH_CHECK(err);
    if (info)
        for (size_t s = 0; s < B; s++) {
            info[s].kf_count = ks[s].kf_count;
            info[s].first = d->list.hdr ? ls[s].first : std::max(0, ks[s].kf_count - 1);
            info[s].held = d->list.hdr ? ls[s].held : 0;
            info[s].overwritten = d->list.hdr ? ls[s].overwritten : 0;
        }
    return slot_read_done(c, slot);
}

int edgehip_keyframe_relocalize_links(edgehip_ctx *c, int seq, int position, int32_t *m_id_f, int32_t *kn_out) {
    EH_ENTER(c);
    auto *d = c->kftrack;
    if (!d) { set_error("keyframe_relocalize_links: key-frame tracking is not enabled"); return EDGEHIP_ERR_STATE; }
    if (!d->reloc_arena) { set_error("keyframe_relocalize_links: no edgehip_keyframe_relocalize call yet"); return EDGEHIP_ERR_STATE; }
    const int M = d->reloc_m;
    if (seq < 0 || seq >= c->plan.nseq || position < 0 || position >= M || !kn_out) { set_error("keyframe_relocalize_links: seq, position or kn_out"); return EDGEHIP_ERR_ARG; }
    const RlLayout y = rl_layout(c, M, std::min(M, kRlMaxPass));
    const uint8_t *base = (const uint8_t *)d->reloc_arena;
    const size_t g = (size_t)seq * M + position;
    EH_CHECK(hipStreamSynchronize(c->stream));
    int32_t kn = -1;
    EH_CHECK(hipMemcpy(&kn, base + y.link_kn + g * 4, 4, hipMemcpyDeviceToHost));
    kn = std::min(kn, c->plan.cap);
    if (kn > 0 && m_id_f) EH_CHECK(hipMemcpy(m_id_f, base + y.links + g * (size_t)c->plan.cap * 4, (size_t)kn * 4, hipMemcpyDeviceToHost));
    *kn_out = kn < 0 ? -1 : kn;
    return 0;
}

int edgehip_keyframe_relocalize_ms(edgehip_ctx *c, double *prepare_ms, double *solve_ms) {
    EH_ENTER(c);
    if (!c->kftrack) { set_error("keyframe_relocalize_ms: key-frame tracking is not enabled"); return EDGEHIP_ERR_STATE; }
    if (prepare_ms) *prepare_ms = c->kftrack->reloc_ms[0];
    if (solve_ms) *solve_ms = c->kftrack->reloc_ms[1];
    return 0;
}

}  // extern "C"
