// keyframe_covis.hip — which key frames of a sequence see the same edges: the reference's kfvo::countMatches (src/mtracklib/kfvo.cpp:18-55,
// with keyframe::reProjectTo, keyframe.h:110-114) and kfvo::kls_on_fov (kfvo.cpp:688-712) over every ordered pair of a sequence's key
// frames — the entries of its key-frame list (keyframe_list.hip) and its current key frame (keyframe_track.hip) — for whole batches.
// Read-only: the kernels below read the key-frame store, the list and (the query form) a ring slot, and write only their own scratch.
//
// Three steps per call, all on the context's stream:
//   gather   every key frame is read ONCE, from its 168-byte records or from the key frame's SoA arrays, and the numbers the rules below
//            read are written to a compact SoA: rho, s_rho (fp64: the match test subtracts and scales them in fp64, Calc_f_J_Complete's
//            `fabs(rho-f_kl.rho)>rho_tol*(f_kl.s_rho+kl.s_rho*rho/kl.rho)` is a double expression), p_m, c_p, u_m, m_m (float2) and n_m:
//            52 B per KeyLine instead of 168.  The pair pass then gathers 52-byte rows, not whole records, M times.
//   field    global_tracker::build_field(edges, radius, min_mod) (global_tracker.cpp:61-105) of a key frame `to`, as a plane of one 32-bit
//            word per pixel.  The reference walks ikl upwards, t over [-radius, radius), and overwrites a cell when |t| <= the cell's dist:
//            a cell ends up with the sample of least |t| and, among those, the greatest ikl, whatever the order.  So every sample does one
//            atomicMin of the key (|t| << 20) | (0xFFFFF - ikl) into a plane cleared to 0xFFFFFFFF (= empty).  20 bits of ikl: max_points <=
//            2^20; 12 bits of |t| without the all-ones pattern: radius <= 4094.  Sample positions are GetIndexRC's (image.h:121-126):
//            round() of u_m * (float)t + c_p in float, no contraction, half away from zero; a sample off the image (or not a number)
//            writes nothing.
//   pairs    one thread per `from` KeyLine, a loop over the `to` planes that are built; the four counts of a pair are 0/1 per lane, summed
//            per wave with a ballot and added by one lane with a vector atomic.
//
// Scratch (allocated on first use, freed with the key frames; M = list capacity + 1 positions per sequence, P = min(M, 8) planes):
//   planes   nseq x P x w x h x 4 B     `to` positions are served P at a time: a pass clears and builds P planes, then scores every
//                                       `from` against them (64 sequences x 8 planes at 752x480: 739 MB; 1024 x 2: 2.96 GB)
//   compact  nseq x (M + 1) x max_points x 52 B   (position M is the query form's ring slot)
//   descriptors, relative poses, counts: (112 + 96 M + 16 M) B x nseq x (M + 1)
//
// The rules, in the reference's types (tests/keyframe_covis_port.py restates them):
//   kl_on_fov, kl_match   p_to = reProjectTo in fp64: u = (p_m.x / rho / zfm, p_m.y / rho / zfm, 1.0 / rho); w = Pose_f * u * K_f + Pos_f;
//            l = Pose_t.T() * (w - Pos_t) / K_t; p_to = (l.x / l.z * zfm, l.y / l.z * zfm, 1 / l.z) (TooN: a dot product per row, 0 += in
//            index order).  p_img = (float)p_to.xy + pp in float; outside when p_img.x < 1 || p_img.y < 1 || p_img.x >= w - 1 ||
//            p_img.y >= h - 1 || p_to.z <= 0; else kl_on_fov counts and the cell ((int)(p_img.y + 0.5), (int)(p_img.x + 0.5)) is looked up
//            with the float instantiation of Calc_f_J_Complete (global_tracker.cpp:115-165): empty, cang < simil_cang (a double holding a
//            float quotient), fabs(n_m / f_n_m - 1) > simil_mod (float), the rho test (double, rho = (float)p_to.z), then fi < max_r with
//            the signed float residual fi.  simil_cang = cos(match_ang) binds to the float overload (kfvo.cpp includes <math.h> through
//            cam_model.h, whose C++ form brings std::cos(float) into the global namespace): cosf, once, on the host.
//   kls_on_fov            q1 = projectImgCordVec((Pose_t.T() * Pose_f) * (u * K_f) + Pose_t.T() * (Pos_f - Pos_t)) in fp64, no K_t;
//            counted unless x < 0 || y < 0 || x >= w || y >= h || q1.z <= 0 with x = (int)(q1.x + 0.5) as x86-64 converts it.
//   guard                 `from` KeyLines whose p_img is not finite: the reference forms a field index from them (out of bounds); here
//            they count as outside the image and no address is formed.  A broken precondition (rho finite and non-zero, finite poses).
// Not reproduced: countMatches leaves the matched field KeyLine's index in kf_from's m_id_f (through Calc_f_J_Complete).  Over many pairs
// only the last pair's survives, and this call writes nothing into a key frame.
#include "keyframe_track.h"

#include <cmath>
#include <cstring>
#include <vector>

namespace edgehip {

constexpr int kCvThreads = 256;
constexpr int kCvMaxPlanes = 8;
constexpr int kCvIklBits = 20;
constexpr uint32_t kCvIklMask = (1u << kCvIklBits) - 1;
constexpr uint32_t kCvEmpty = 0xFFFFFFFFu;
constexpr int kCvMaxRadius = 4094;   // (4095 << 20) | kCvIklMask would be kCvEmpty

struct CvCompact {           // [nseq * (M + 1)][cap] each
    double *rho, *s_rho;
    float2 *p_m, *c_p, *u_m, *m_m;
    float *n_m;
};

struct CvArgs {
    CvCompact k;
    CvKf *desc;                    // [nseq][M + 1]
    double *rel;                   // [nseq][M][M + 1][12]: Pose_t.T() * Pose_f, Pose_t.T() * (Pos_f - Pos_t)
    uint32_t *planes;              // [nseq][P][n]
    edgehip_kf_pair_count *out;    // [nseq][M][M], or [nseq][M] (the query form)
    int nseq, M, P, cap, w, h;
    int radius;
    float min_mod, simil_mod, simil_cang, rho_tol, max_r;
    float ppx, ppy;
    double zfm;
    int query;                     // 0: all pairs; 1: position M against every key frame
};

__global__ void k_cv_desc(CvArgs a, const KfSeq *__restrict__ ks, KfListDev l, const int32_t *__restrict__ slot_kn,
                          const edgehip_kf_pose *__restrict__ pose_in, const SeqDev *__restrict__ seqs, const edgehip_nav *__restrict__ nav) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.nseq * (a.M + 1)) return;
    const int seq = g / (a.M + 1), pos = g % (a.M + 1);
    a.desc[g] = kf_position(seq, pos, a.M, a.cap, ks, l, slot_kn, pose_in, seqs, nav);
}

// per (seq, to, from): kls_on_fov's BRelRot / BRelPos (kfvo.cpp:692-693), and the pair's counts start at 0, or are -1 for good
__global__ void k_cv_init(CvArgs a) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    const int M1 = a.M + 1;
    if (g >= a.nseq * a.M * M1) return;
    const int from = g % M1, to = (g / M1) % a.M, seq = g / (M1 * a.M);
    const CvKf &t = a.desc[(size_t)seq * M1 + to], &f = a.desc[(size_t)seq * M1 + from];
    double *r = a.rel + (size_t)g * 12;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) {
            double s = 0;
            for (int k = 0; k < 3; k++) s += t.Pose[3 * k + i] * f.Pose[3 * k + j];
            r[3 * i + j] = s;
        }
        double s = 0;
        for (int k = 0; k < 3; k++) s += t.Pose[3 * k + i] * (f.Pos[k] - t.Pos[k]);
        r[9 + i] = s;
    }
    const int v = (t.kn >= 0 && f.kn >= 0) ? 0 : -1;
    edgehip_kf_pair_count z = {v, v, v, v};
    if (!a.query) { if (from < a.M) a.out[((size_t)seq * a.M + to) * a.M + from] = z; }
    else if (from == a.M) a.out[(size_t)seq * a.M + to] = z;
}

__global__ __launch_bounds__(kCvThreads) void k_cv_gather(CvArgs a, KfListDev l, const KlSoA *__restrict__ kf_kl, const KlSoA *__restrict__ slot_kl) {
    const int seq = blockIdx.z, pos = blockIdx.y, i = blockIdx.x * kCvThreads + threadIdx.x;
    const size_t g = (size_t)seq * (a.M + 1) + pos;
    const CvKf &d = a.desc[g];
    if (i >= d.kn) return;
    const size_t o = g * a.cap + i;
    if (d.src >= 0) {
        const edgehip_keyline *r = reinterpret_cast<const edgehip_keyline *>(l.rec + ((size_t)seq * l.capacity + d.src) * l.stride) + i;
        a.k.rho[o] = r->rho; a.k.s_rho[o] = r->s_rho;
        a.k.p_m[o] = make_float2(r->p_m[0], r->p_m[1]); a.k.c_p[o] = make_float2(r->c_p[0], r->c_p[1]);
        a.k.u_m[o] = make_float2(r->u_m[0], r->u_m[1]); a.k.m_m[o] = make_float2(r->m_m[0], r->m_m[1]);
        a.k.n_m[o] = r->n_m;
    } else {
        const KlSoA &s = d.src == -1 ? kf_kl[seq] : slot_kl[seq];
        a.k.rho[o] = s.rho[i]; a.k.s_rho[o] = s.s_rho[i];
        a.k.p_m[o] = s.p_m[i]; a.k.c_p[o] = s.c_p[i]; a.k.u_m[o] = s.u_m[i]; a.k.m_m[o] = s.m_m[i];
        a.k.n_m[o] = s.n_m[i];
    }
}

// The planes of the positions [t0, t0 + P) (cleared by the caller).  A wave owns 64 consecutive KeyLines and takes them one after the other with
// its lanes along t (lane l: t = -radius + l, + 64, ...): the atomics of a wave-instruction then go to neighbouring pixels of one segment —
// one or a few cache lines for a flat segment — instead of 64 unrelated ones (a lane per KeyLine measured 1.6 x slower).
__global__ __launch_bounds__(kCvThreads) void k_cv_field(CvArgs a, int t0) {
    const int seq = blockIdx.z, pl = blockIdx.y, to = t0 + pl, i = blockIdx.x * kCvThreads + threadIdx.x, lane = threadIdx.x & 63;
    if (to >= a.M) return;
    const size_t g = (size_t)seq * (a.M + 1) + to;
    const int kn = a.desc[g].kn;
    if ((int)(blockIdx.x * kCvThreads + (threadIdx.x & ~63)) >= kn) return;   // wave-uniform
    const bool live = i < kn;
    const size_t o = g * a.cap + (live ? i : 0);
    const bool use = live && !(a.min_mod > 0 && a.k.n_m[o] < a.min_mod);
    const float2 u = a.k.u_m[o], c = a.k.c_p[o];   // (lanes past the list read KeyLine 0 and are not used)
    uint32_t *plane = a.planes + ((size_t)seq * a.P + pl) * ((size_t)a.w * a.h);
    const float fw = (float)a.w, fh = (float)a.h;
    unsigned long long todo = __ballot(use);
    while (todo) {
        const int j = __builtin_ctzll(todo);
        todo &= todo - 1;
        const float ux = __shfl(u.x, j, 64), uy = __shfl(u.y, j, 64), cx = __shfl(c.x, j, 64), cy = __shfl(c.y, j, 64);
        const uint32_t low = kCvIklMask - (uint32_t)((i - lane) + j);
        for (int t = -a.radius + lane; t < a.radius; t += 64) {
            const float x = roundf(ux * (float)t + cx), y = roundf(uy * (float)t + cy);
            if (!(x >= 0.f && x < fw && y >= 0.f && y < fh)) continue;   // off the image, or NaN; else 0 <= (int)x < w, 0 <= (int)y < h
            atomicMin(plane + (size_t)(int)y * a.w + (int)x, ((uint32_t)abs(t) << kCvIklBits) | low);
        }
    }
}

// `from` positions from0 + blockIdx.y against the planes of [t0, t0 + P)
__global__ __launch_bounds__(kCvThreads) void k_cv_pairs(CvArgs a, int t0, int from0) {
    const int seq = blockIdx.z, from = from0 + blockIdx.y, r0 = blockIdx.x * kCvThreads;
    const int M1 = a.M + 1;
    const size_t gf = (size_t)seq * M1 + from;
    const CvKf &f = a.desc[gf];
    if (f.kn <= r0) return;                      // block-uniform: absent (-1), or the list ends before this tile
    const int i = r0 + threadIdx.x, lane = threadIdx.x & 63;
    const bool live = i < f.kn;
    const size_t o = gf * a.cap + (live ? i : 0);
    const double rho = a.k.rho[o], s_rho = a.k.s_rho[o];
    const float2 p_m = a.k.p_m[o], m_m = a.k.m_m[o];
    const float n_m = a.k.n_m[o];
    // camera.unprojectHomCordVec (cam_model.h:163-169), Local2WorldScaled (keyframe.h:101-103), and kls_on_fov's p0 = u * K
    double u[3], wp[3], p0[3];
    u[0] = (double)p_m.x / rho / a.zfm; u[1] = (double)p_m.y / rho / a.zfm; u[2] = 1.0 / rho;
    for (int r = 0; r < 3; r++) {
        double s = 0;
        s += f.Pose[3 * r] * u[0]; s += f.Pose[3 * r + 1] * u[1]; s += f.Pose[3 * r + 2] * u[2];
        wp[r] = s * f.K + f.Pos[r];
        p0[r] = u[r] * f.K;
    }
    const float wm1 = (float)(a.w - 1), hm1 = (float)(a.h - 1);
    const int t1 = min(t0 + a.P, a.M);
    for (int to = t0; to < t1; to++) {
        const size_t gt = (size_t)seq * M1 + to;
        const CvKf &t = a.desc[gt];
        if (t.kn < 0) continue;                  // uniform
        bool on_fov = false, match = false, on_kls = false, bad = false;
        if (live) {
            // World2LocalScaled (keyframe.h:98-100), projectHomCordVec (cam_model.h:146-152)
            double d[3], lc[3];
            for (int r = 0; r < 3; r++) d[r] = wp[r] - t.Pos[r];
            for (int r = 0; r < 3; r++) {
                double s = 0;
                s += t.Pose[r] * d[0]; s += t.Pose[3 + r] * d[1]; s += t.Pose[6 + r] * d[2];
                lc[r] = s / t.K;
            }
            const double px = lc[0] / lc[2] * a.zfm, py = lc[1] / lc[2] * a.zfm, pz = 1 / lc[2];
            const float ix = (float)px + a.ppx, iy = (float)py + a.ppy;
            bad = !(isfinite(ix) && isfinite(iy));
            if (!bad && !(ix < 1 || iy < 1 || ix >= wm1 || iy >= hm1 || pz <= 0)) {
                on_fov = true;
                const int x = (int)((double)ix + 0.5), y = (int)((double)iy + 0.5);   // 1 <= x <= w - 1, 1 <= y <= h - 1
                const uint32_t key = a.planes[((size_t)seq * a.P + (to - t0)) * ((size_t)a.w * a.h) + (size_t)y * a.w + x];
                if (key != kCvEmpty) {
                    const size_t q = gt * a.cap + (kCvIklMask - (key & kCvIklMask));   // an index the field kernel wrote: < t.kn
                    const float2 fm = a.k.m_m[q];
                    const float fn = a.k.n_m[q];
                    const double f_rho = a.k.rho[q], f_s_rho = a.k.s_rho[q];
                    const double cang = (double)((m_m.x * fm.x + m_m.y * fm.y) / n_m);
                    const float frho = (float)pz;
                    const bool rej = cang < (double)a.simil_cang || fabsf(n_m / fn - 1) > a.simil_mod ||
                                     fabs((double)frho - f_rho) > (double)a.rho_tol * (f_s_rho + s_rho * (double)frho / rho);
                    if (!rej) {
                        const float2 fc = a.k.c_p[q], fu = a.k.u_m[q];
                        const float dx = ix - fc.x, dy = iy - fc.y;
                        const float fi = dx * fu.x + dy * fu.y;
                        match = fi < a.max_r;
                    }
                }
            }
            // kls_on_fov (kfvo.cpp:696-707), projectImgCordVec (cam_model.h:154-160)
            const double *R = a.rel + (((size_t)seq * a.M + to) * M1 + from) * 12;
            double v[3];
            for (int r = 0; r < 3; r++) {
                double s = 0;
                s += R[3 * r] * p0[0]; s += R[3 * r + 1] * p0[1]; s += R[3 * r + 2] * p0[2];
                v[r] = s + R[9 + r];
            }
            const double qx = v[0] / v[2] * a.zfm + (double)a.ppx, qy = v[1] / v[2] * a.zfm + (double)a.ppy, qz = 1 / v[2];
            const int x = x86_cvttsd2si(qx + 0.5), y = x86_cvttsd2si(qy + 0.5);
            on_kls = !(x < 0 || y < 0 || x >= a.w || y >= a.h || qz <= 0);
        }
        const int c0 = __popcll(__ballot(on_fov)), c1 = __popcll(__ballot(match)), c2 = __popcll(__ballot(on_kls)), c3 = __popcll(__ballot(bad));
        if (lane == 0) {
            edgehip_kf_pair_count *dst = a.query ? a.out + (size_t)seq * a.M + to : a.out + ((size_t)seq * a.M + to) * a.M + from;
            if (c0) atomicAdd(&dst->kl_on_fov, c0);
            if (c1) atomicAdd(&dst->kl_match, c1);
            if (c2) atomicAdd(&dst->kls_on_fov, c2);
            if (c3) atomicAdd(&dst->guard, c3);
        }
    }
}

}  // namespace edgehip

using namespace edgehip;

namespace {
struct CvLayout {
    size_t planes, rho, s_rho, p_m, c_p, u_m, m_m, n_m, desc, rel, out, pose, state, total;
};
CvLayout cv_layout(size_t B, size_t M, size_t P, size_t cap, size_t n) {
    CvLayout y;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; };
    const size_t kl = B * (M + 1) * cap;
    y.planes = take(B * P * n * 4);
    y.rho = take(kl * 8); y.s_rho = take(kl * 8);
    y.p_m = take(kl * 8); y.c_p = take(kl * 8); y.u_m = take(kl * 8); y.m_m = take(kl * 8);
    y.n_m = take(kl * 4);
    y.desc = take(B * (M + 1) * sizeof(CvKf));
    y.rel = take(B * M * (M + 1) * 12 * 8);
    y.out = take(B * M * M * sizeof(edgehip_kf_pair_count));
    y.pose = take(B * sizeof(edgehip_kf_pose));
    y.total = at;
    return y;
}
}  // namespace

void edgehip::kf_covis_free(edgehip_ctx *c) {
    auto *d = c->kftrack;
    if (!d || !d->covis_arena) return;
    (void)hipFree(d->covis_arena);
    d->covis_arena = nullptr; d->covis_m = 0;
    d->covis_ms[0] = d->covis_ms[1] = 0;
}

static int cv_run(edgehip_ctx *c, const char *who, int slot, const edgehip_kf_pose *pose, const edgehip_kf_covis_args *args,
                  edgehip_kf_pair_count *out, edgehip_kf_list_info *info) {
    auto *d = c->kftrack;
    if (!d) { set_error(std::string(who) + ": key-frame tracking is not enabled (edgehip_keyframe_track_enable)"); return EDGEHIP_ERR_STATE; }
    if (!args || !out) { set_error(std::string(who) + ": null args or out"); return EDGEHIP_ERR_ARG; }
    if (args->field_radius < 1 || args->field_radius > kCvMaxRadius) {
        set_error(std::string(who) + ": field_radius must be in [1, 4094] (12 bits of the field's packed key)");
        return EDGEHIP_ERR_ARG;
    }
    if (c->plan.cap > (int)kCvIklMask + 1) { set_error(std::string(who) + ": max_points above 2^20 (20 bits of the field's packed key)"); return EDGEHIP_ERR_ARG; }
    const bool query = slot != -1;
    if (query && (slot < 0 || slot >= c->plan.nslots)) { set_error(std::string(who) + ": slot out of range"); return EDGEHIP_ERR_ARG; }
    const size_t B = c->plan.nseq, n = (size_t)c->plan.w * c->plan.h, cap = c->plan.cap;
    const int M = d->list.hdr ? d->list.capacity + 1 : 1, P = std::min(M, kCvMaxPlanes);
    const CvLayout y = cv_layout(B, M, P, cap, n);
    if (d->covis_arena && d->covis_m != M) {   // the list was enabled, freed or resized since
        EH_CHECK(hipStreamSynchronize(c->stream));
        kf_covis_free(c);
    }
    if (!d->covis_arena) {
        void *p = nullptr;
        if (hipMalloc(&p, y.total) != hipSuccess) {
            (void)hipGetLastError();
            set_error(std::string(who) + ": scratch allocation failed (planes nseq x min(M, 8) x w x h x 4 B, compact KeyLines nseq x (M + 1) x max_points x 52 B)");
            return EDGEHIP_ERR_MEMORY;
        }
        d->covis_arena = p; d->covis_m = M;
    }
    if (query) {
        if (int e = rot_materialize_enqueue(c, slot)) return e;   // the slot's KeyLines as edgehip_download_keylines returns them
        if (int e = order_bc_after_a(c)) return e;
    }
    uint8_t *base = (uint8_t *)d->covis_arena;
    CvArgs a;
    a.k.rho = (double *)(base + y.rho); a.k.s_rho = (double *)(base + y.s_rho);
    a.k.p_m = (float2 *)(base + y.p_m); a.k.c_p = (float2 *)(base + y.c_p); a.k.u_m = (float2 *)(base + y.u_m); a.k.m_m = (float2 *)(base + y.m_m);
    a.k.n_m = (float *)(base + y.n_m);
    a.desc = (CvKf *)(base + y.desc); a.rel = (double *)(base + y.rel); a.planes = (uint32_t *)(base + y.planes);
    a.out = (edgehip_kf_pair_count *)(base + y.out);
    a.nseq = (int)B; a.M = M; a.P = P; a.cap = (int)cap; a.w = c->plan.w; a.h = c->plan.h;
    a.radius = args->field_radius; a.min_mod = args->field_min_mod;
    a.simil_mod = args->match_mod; a.simil_cang = cosf(args->match_ang); a.rho_tol = args->rho_tol; a.max_r = args->max_r;
    a.ppx = c->plan.ppx; a.ppy = c->plan.ppy; a.zfm = c->plan.zfm;
    a.query = query;
    edgehip_kf_pose *pose_dev = nullptr;
    if (query && pose) {   // (pageable memory: the copy has left the caller's array when the call returns; the call synchronises anyway)
        pose_dev = (edgehip_kf_pose *)(base + y.pose);
        EH_CHECK(hipMemcpyAsync(pose_dev, pose, sizeof(edgehip_kf_pose) * B, hipMemcpyHostToDevice, c->stream));
    }
    hipStream_t st = c->stream;
    const int M1 = M + 1;
    hipLaunchKernelGGL(k_cv_desc, dim3((unsigned)((B * M1 + 63) / 64)), dim3(64), 0, st, a, (const KfSeq *)d->ks, d->list,
                       (const int32_t *)(query ? c->kn_slot + (size_t)slot * B : nullptr), (const edgehip_kf_pose *)pose_dev,
                       (const SeqDev *)c->seq, (const edgehip_nav *)c->nav_dev);
    EH_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cv_init, dim3((unsigned)((B * M * M1 + 63) / 64)), dim3(64), 0, st, a);
    EH_LAUNCH_CHECK();
    const unsigned tiles = (unsigned)((cap + kCvThreads - 1) / kCvThreads);
    std::vector<hipEvent_t> ev;
    auto mark = [&]() -> hipError_t {
        hipEvent_t e = nullptr;
        hipError_t r = hipEventCreate(&e);
        if (r != hipSuccess) return r;
        ev.push_back(e);
        return hipEventRecord(e, st);
    };
    auto drop = [&]() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); ev.clear(); };
    hipError_t err = mark();
    if (err == hipSuccess) {
        hipLaunchKernelGGL(k_cv_gather, dim3(tiles, M1, (unsigned)B), dim3(kCvThreads), 0, st, a, d->list, (const KlSoA *)d->kl_dev,
                           (const KlSoA *)(query ? kldev(c, slot) : d->kl_dev));
        err = hipGetLastError();
    }
    for (int t0 = 0; t0 < M && err == hipSuccess; t0 += P) {
        err = hipMemsetAsync(a.planes, 0xFF, B * P * n * 4, st);
        if (err != hipSuccess) break;
        hipLaunchKernelGGL(k_cv_field, dim3(tiles, P, (unsigned)B), dim3(kCvThreads), 0, st, a, t0);
        if ((err = hipGetLastError()) != hipSuccess) break;
        if ((err = mark()) != hipSuccess) break;
        hipLaunchKernelGGL(k_cv_pairs, dim3(tiles, query ? 1 : M, (unsigned)B), dim3(kCvThreads), 0, st, a, t0, query ? M : 0);
        if ((err = hipGetLastError()) != hipSuccess) break;
        err = mark();
    }
    if (err != hipSuccess) { drop(); EH_CHECK(err); }
    std::vector<KfListSeq> ls(B);
    std::vector<KfSeq> ks(info ? B : 0);
    err = hipMemcpyAsync(out, a.out, sizeof(edgehip_kf_pair_count) * B * M * (query ? 1 : M), hipMemcpyDeviceToHost, st);
    if (err == hipSuccess && info) {
        if (d->list.hdr) err = hipMemcpyAsync(ls.data(), d->list.ls, sizeof(KfListSeq) * B, hipMemcpyDeviceToHost, st);
        if (err == hipSuccess) err = hipMemcpyAsync(ks.data(), d->ks, sizeof(KfSeq) * B, hipMemcpyDeviceToHost, st);
    }
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    if (err == hipSuccess) {   // events 0, 1: gather + first field; then (pairs, field) alternate
        d->covis_ms[0] = d->covis_ms[1] = 0;
        for (size_t j = 0; j + 1 < ev.size() && err == hipSuccess; j++) {
            float ms = 0;
            err = hipEventElapsedTime(&ms, ev[j], ev[j + 1]);
            d->covis_ms[j & 1] += ms;
        }
    }
    drop();
    EH_CHECK(err);
    if (info)
        for (size_t s = 0; s < B; s++) {
            info[s].kf_count = ks[s].kf_count;
            info[s].first = d->list.hdr ? ls[s].first : std::max(0, ks[s].kf_count - 1);
            info[s].held = d->list.hdr ? ls[s].held : 0;
            info[s].overwritten = d->list.hdr ? ls[s].overwritten : 0;
        }
    if (query) return slot_read_done(c, slot);
    return 0;
}

int edgehip_keyframe_covisibility(edgehip_ctx *c, const edgehip_kf_covis_args *args, edgehip_kf_pair_count *out, edgehip_kf_list_info *info) {
    EH_ENTER(c);
    return cv_run(c, "keyframe_covisibility", -1, nullptr, args, out, info);
}

int edgehip_keyframe_covisibility_slot(edgehip_ctx *c, int slot, const edgehip_kf_pose *pose, const edgehip_kf_covis_args *args,
                                       edgehip_kf_pair_count *out, edgehip_kf_list_info *info) {
    EH_ENTER(c);
    if (slot == -1) { set_error("keyframe_covisibility_slot: slot out of range"); return EDGEHIP_ERR_ARG; }
    return cv_run(c, "keyframe_covisibility_slot", slot, pose, args, out, info);
}

int edgehip_keyframe_covisibility_ms(edgehip_ctx *c, double *field_ms, double *pair_ms) {
    EH_ENTER(c);
    if (!c->kftrack) { set_error("keyframe_covisibility_ms: key-frame tracking is not enabled"); return EDGEHIP_ERR_STATE; }
    if (field_ms) *field_ms = c->kftrack->covis_ms[0];
    if (pair_ms) *pair_ms = c->kftrack->covis_ms[1];
    return 0;
}
