// surface_integrate.hip — REBVO's cross-view surface integration (src/visualizer/surface_integrator.cpp, app/kf_visualizer/main.cpp:110-116,
// 192, 201) over a store of filled depth grids ("views": grid + Pose, Pos, K), restated as two order-free passes over a voxel plane:
//   k_sv_bounds  analizeSpaceSize (surface_integrator.cpp:32-68): per view the min / max of Local2WorldScaled(get3DPos(x, y)); the host
//                folds the views (min and max do not depend on the order).
//   k_sv_clear   zeroes the voxel plane (16-B stores).
//   k_sv_rays    rayCutSurface (:235-266): one ray per thread, pos += unit(dir) * min_block accumulated serially in fp64 as the reference
//                does; every step records the casting view in the voxel it lands in.
//   k_sv_test    fillKFList's sample walk (:167-229) per cell, in the reference's order (float accumulators, double increments), looked up in
//                the plane instead of registered in it: the cell is hidden iff some sample's voxel holds a view other than the cell's own.
// The reference keeps a list of surface cells per voxel and lets every ray step clear the `visibility` of the cells of other views it
// finds there.  Visibility only falls, so cell c of view A ends hidden iff some voxel holds both a fill sample of c and a ray step of a
// casting view B != A: the lists are not needed, only which views' rays crossed a voxel.
//
// Voxel word (4 B): 0 = no ray; bits 0..30 = largest casting view id + 1 seen so far; bit 31 = "rays of two or more views".  A ray step
// does atomicMax(word, id + 1) and, if the value it replaced was another view's (non-zero, not its own, bit 31 clear), atomicOr(bit 31).
// Whatever the order of arrival, the first step of the second distinct view sees the first one's id and sets bit 31 (from then on the
// atomicMax changes nothing), so "word != 0 and (bit 31 or id != A + 1)" — the test for view A — does not depend on the order.  An
// agent-scope load in front skips both atomics where the word already says so (every ray of a view starts in the camera's voxel).
//   k_sv_ray_cross  SurfaceInt::checkDFRayCrossExaustive (:70-116): the same question without the voxel plane, every cell of a target
//                view against every ray of a hidder view, many ordered pairs of views per launch (see the kernel).
// fp64 as the reference uses it; '/' and sqrt are the compiler's correctly rounded operations; -ffp-contract=off keeps products and sums
// separately rounded.
#include "ctx.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace edgehip {

constexpr int kSvThreads = 256;
constexpr int kSvMaxViews = 1024;                // the stored / casting sets travel as bit masks in the kernel arguments
constexpr int kSvMaskWords = kSvMaxViews / 64;
constexpr unsigned kSvMulti = 0x80000000u;

struct SvMask {
    uint64_t w[kSvMaskWords];
    __host__ __device__ bool has(int v) const { return (w[v >> 6] >> (v & 63)) & 1; }
};

struct SvGeom {                 // camera and grid of the context
    int gw, gh, bw, bh;
    float ppx, ppy;
    double zfm;
};

struct SvBox {                  // OcGrid (surface_integrator.cpp:120-132)
    double origin[3], block[3], min_block;
    unsigned n[3];
};

struct SvStore {
    const double *rho, *s_rho;  // [cap][G]
    const double *pose;         // [cap][13]: Pose (row-major 3x3), Pos, K
    uint8_t *vis;               // [cap][G]
};

// keyframe::Local2WorldScaled (keyframe.h:101-103): Pose * p * K + Pos; TooN's Matrix * Vector is a dot product per row (result = 0, += in
// index order), then the scalar product, then the sum.
__device__ __forceinline__ void sv_l2w(const double *M, const double p[3], double o[3]) {
    for (int i = 0; i < 3; i++) {
        double s = 0;
        s += M[3 * i] * p[0];
        s += M[3 * i + 1] * p[1];
        s += M[3 * i + 2] * p[2];
        o[i] = s * M[12] + M[9 + i];
    }
}

// get3DPos / get3DPosShiftRho (depth_filler.h:115-131) with the divisor given: the cell centre ((float)x + 0.5) * bw — a double product —
// rounded to float, minus the principal point in float, / zfm in double, / r in double.
__device__ __forceinline__ void sv_cell_point(int x, int y, double r, const SvGeom &g, double P[3]) {
    const float ix = (float)(((double)(float)x + 0.5) * (double)g.bw);
    const float iy = (float)(((double)(float)y + 0.5) * (double)g.bh);
    const float hx = ix - g.ppx, hy = iy - g.ppy;
    P[0] = ((double)hx / g.zfm) / r;
    P[1] = ((double)hy / g.zfm) / r;
    P[2] = 1.0 / r;
}

// OcGrid::wordl2Index (surface_integrator.h:66-69): (p - origin)[i] / block[i] truncated per axis.  A quotient that is negative, not
// finite or >= n on any axis is outside the box: the point is dropped (the reference indexes with the wrapped conversion).  q[] is
// left for the caller (the ray's early exit).
__device__ __forceinline__ bool sv_voxel(const double p[3], const SvBox &b, size_t &idx, double q[3]) {
    bool in = true;
    unsigned u[3];
    for (int i = 0; i < 3; i++) {
        q[i] = (p[i] - b.origin[i]) / b.block[i];
        const bool ok = q[i] >= 0.0 && q[i] < (double)b.n[i];
        in = in && ok;
        u[i] = ok ? (unsigned)q[i] : 0u;
    }
    idx = (size_t)u[2] * ((size_t)b.n[0] * b.n[1]) + (size_t)u[1] * b.n[0] + u[0];
    return in;
}

__global__ __launch_bounds__(kSvThreads) void k_sv_bounds(SvStore st, SvGeom g, SvMask stored, double *part) {
    __shared__ double red[6][kSvThreads];
    const int view = blockIdx.x, tid = threadIdx.x, G = g.gw * g.gh;
    if (!stored.has(view)) return;
    const double *rho = st.rho + (size_t)view * G, *M = st.pose + (size_t)view * 13;
    double mn[3] = {1e20, 1e20, 1e20}, mx[3] = {1e-20, 1e-20, 1e-20};   // the reference's starts (:36-38)
    for (int c = tid; c < G; c += kSvThreads) {
        double P[3], W[3];
        sv_cell_point(c % g.gw, c / g.gw, rho[c], g, P);
        sv_l2w(M, P, W);
        for (int i = 0; i < 3; i++) {
            if (W[i] < mn[i]) mn[i] = W[i];   // util::keep_min / keep_max: never take a NaN
            if (W[i] > mx[i]) mx[i] = W[i];
        }
    }
    for (int i = 0; i < 3; i++) { red[i][tid] = mn[i]; red[3 + i][tid] = mx[i]; }
    __syncthreads();
    for (int s = kSvThreads / 2; s > 0; s >>= 1) {
        if (tid < s)
            for (int i = 0; i < 3; i++) {
                if (red[i][tid + s] < red[i][tid]) red[i][tid] = red[i][tid + s];
                if (red[3 + i][tid + s] > red[3 + i][tid]) red[3 + i][tid] = red[3 + i][tid + s];
            }
        __syncthreads();
    }
    if (tid < 6) part[view * 6 + tid] = red[tid][0];
}

__global__ __launch_bounds__(kSvThreads) void k_sv_clear(uint4 *plane16, size_t n16, unsigned *tail, int ntail) {
    const size_t stride = (size_t)gridDim.x * kSvThreads;
    for (size_t i = (size_t)blockIdx.x * kSvThreads + threadIdx.x; i < n16; i += stride) plane16[i] = make_uint4(0, 0, 0, 0);
    if (blockIdx.x == 0 && (int)threadIdx.x < ntail) tail[threadIdx.x] = 0;
}

__global__ __launch_bounds__(kSvThreads) void k_sv_rays(SvStore st, SvGeom g, SvBox b, SvMask cast, unsigned *plane) {
    const int view = blockIdx.y, G = g.gw * g.gh;
    const int c = blockIdx.x * kSvThreads + threadIdx.x;
    if (!cast.has(view) || c >= G) return;
    const double *M = st.pose + (size_t)view * 13;
    const double zero[3] = {0, 0, 0};
    double ro[3], rp[3], P[3], d[3];
    sv_l2w(M, zero, ro);
    sv_cell_point(c % g.gw, c / g.gw, st.rho[(size_t)view * G + c] + st.s_rho[(size_t)view * G + c], g, P);
    sv_l2w(M, P, rp);
    double nn = 0;
    for (int i = 0; i < 3; i++) d[i] = rp[i] - ro[i];
    for (int i = 0; i < 3; i++) nn += d[i] * d[i];
    const double nrm = sqrt(nn), inv = 1 / nrm;   // TooN::norm; unit(v) = v * (1 / sqrt(v * v))
    double step[3], pos[3];
    for (int i = 0; i < 3; i++) { step[i] = d[i] * inv * b.min_block; pos[i] = ro[i]; }
    // int step_num = norm / min_block: cvttsd2si answers INT_MIN for a NaN or a quotient past the int range — no steps
    const int steps = x86_cvttsd2si(nrm / b.min_block);
    const unsigned me = (unsigned)view + 1;
    size_t last = ~(size_t)0;
    for (int k = 0; k < steps; k++) {
        size_t idx;
        double q[3];
        if (sv_voxel(pos, b, idx, q)) {
            if (idx != last) {
                last = idx;
                unsigned *w = plane + idx;
                const unsigned cur = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (cur != me && !(cur & kSvMulti)) {
                    const unsigned old = atomicMax(w, me);
                    if (old != 0 && old != me && !(old & kSvMulti)) atomicOr(w, kSvMulti);
                }
            }
        } else {
            // pos[i] only ever moves the way of step[i] (adding one constant is monotone in floating point), and so does q[i]: a ray that is
            // past the box on an axis in its own direction, or whose position is no number, never comes back.  Every later step would be
            // dropped as well.
            bool gone = false;
            for (int i = 0; i < 3; i++)
                gone = gone || !(q[i] == q[i]) || (q[i] >= (double)b.n[i] && !(step[i] < 0)) || (q[i] < 0.0 && !(step[i] > 0));
            if (gone) break;
        }
        for (int i = 0; i < 3; i++) pos[i] += step[i];
    }
}

// getImg3DPos's index terms of one float coordinate (depth_filler.h:140-148): float x_histo = x / (float)b - 0.5 (a float division, a
// double subtraction, back to float); f / c = floor / ceil clamped to [0, n-1] in double, then int; d = x_histo - f in float.
__device__ __forceinline__ void sv_terms(float x, int b, int n, int &f, int &c, float &d) {
    const float xh = (float)((double)(x / (float)b) - 0.5);
    const float fl = floorf(xh), ce = ceilf(xh);
    f = fl < 0.0f ? 0 : (fl > (float)(n - 1) ? n - 1 : (int)fl);
    c = ce < 0.0f ? 0 : (ce > (float)(n - 1) ? n - 1 : (int)ce);
    d = xh - (float)f;
}

__global__ __launch_bounds__(kSvThreads) void k_sv_test(SvStore st, SvGeom g, SvBox b, SvMask stored, const unsigned *plane, int accumulate) {
    const int view = blockIdx.y, G = g.gw * g.gh;
    const int c = blockIdx.x * kSvThreads + threadIdx.x;
    if (!stored.has(view) || c >= G) return;
    const double *rho = st.rho + (size_t)view * G, *M = st.pose + (size_t)view * 13;
    uint8_t *vis = st.vis + (size_t)view * G;
    const unsigned me = (unsigned)view + 1;
    const unsigned gx = c % g.gw, gy = c / g.gw;
    bool hidden = false;
    // fillKFList (:183-196): the cell's projected rectangle in voxels gives the sample step in pixels
    const double min_rho = rho[c] / M[12];
    if (min_rho > 0.0 && min_rho < INFINITY) {   // else: no samples (the reference's loop does not end when the step is 0)
        const double rect_x = (double)g.bw / g.zfm / min_rho, rect_y = (double)g.bh / g.zfm / min_rho;
        const double qx = rect_x / b.min_block, qy = rect_y / b.min_block;
        const double snx = qx < 1.0 ? 1.0 : qx, sny = qy < 1.0 ? 1.0 : qy;   // std::max(q, 1.0)
        const double step_x = (double)g.bw / snx, step_y = (double)g.bh / sny;
        const float x0 = (float)(gx * (unsigned)g.bw), x1 = (float)((gx + 1) * (unsigned)g.bw);
        const float y1 = (float)((gy + 1) * (unsigned)g.bh);
        bool walk = step_x > 0.0 && step_y > 0.0;
        for (float iy = (float)(gy * (unsigned)g.bh); walk && iy < y1;) {
            int yf, yc;
            float dy;
            sv_terms(iy, g.bh, g.gh, yf, yc, dy);
            const double *rf = rho + yf * g.gw, *rc = rho + yc * g.gw;
            for (float ix = x0; ix < x1;) {
                int xf, xc;
                float dx;
                sv_terms(ix, g.bw, g.gw, xf, xc, dx);
                const float r00 = (float)rf[xf], r10 = (float)rf[xc], r01 = (float)rc[xf], r11 = (float)rc[xc];
                const float r = r00 * (1 - dx) * (1 - dy) + r10 * dx * (1 - dy) + r01 * (1 - dx) * dy + r11 * dx * dy;   // depth_filler.h:156
                const float hx = ix - g.ppx, hy = iy - g.ppy;
                double P[3] = {((double)hx / g.zfm) / (double)r, ((double)hy / g.zfm) / (double)r, 1.0 / (double)r}, W[3], q[3];
                sv_l2w(M, P, W);
                size_t idx;
                if (sv_voxel(W, b, idx, q)) {
                    const unsigned w = plane[idx];
                    if (w != 0 && ((w & kSvMulti) || w != me)) { hidden = true; walk = false; break; }   // visibility only falls: the rest cannot matter
                }
                const float nx = (float)((double)ix + step_x);   // float i_x += double step
                if (!(nx > ix)) { walk = false; break; }         // an accumulator that no longer advances never ends in the reference
                ix = nx;
            }
            const float ny = (float)((double)iy + step_y);
            if (!(ny > iy)) break;
            iy = ny;
        }
    }
    vis[c] = accumulate ? (uint8_t)(vis[c] && !hidden) : (uint8_t)!hidden;
}

// SurfaceInt::checkDFRayCrossExaustive(target, hidder) (surface_integrator.cpp:70-116) for a list of ordered pairs of views.  A target
// cell is hidden when some hidder ray passes it closer than the cell's bubble (norm((point - ray_orig) ^ ray_versor) < buble_size, :98-100)
// and the cell lies in front of the hidder's surface on that ray (0 < (point - ray_orig) * ray_versor < dist, :101-102).  The reference
// recomputes everything inside its four loops; what depends on the hidder cell alone (ray_versor, dist), on the pair alone (ray_orig) or
// on the target cell alone (point, buble_size, point - ray_orig) is formed once here, by the same operations in the same order.
//
// blockIdx.x = pair, blockIdx.y = 256 target cells, one per thread, in registers.  The block builds the hidder's rays a tile of 256 at a
// time in LDS (one ray per thread); every lane then reads the same ray, a broadcast.  Visibility only falls, so a lane that finds its
// cell hidden, or found it hidden already (an earlier call under accumulate, or another pair of this launch: any 0 read here is a
// final value), has nothing left to find: a wave leaves the ray loop when all its lanes are so, the block when all its waves are.
//
// The square root of :98 is taken only where it can decide: with n2 the squared norm, sqrt(n2) < b is certain when n2 < b * b * (1 - 1e-6)
// and impossible when n2 > b * b * (1 + 1e-6) (sqrt is monotone and correctly rounded; the margins are ten orders of magnitude above
// the rounding of b * b and of the root).  In between, for a NaN, and for every bubble that is not a positive number whose square is
// far from the subnormals and from infinity, the reference's own comparison decides.
struct SvRay { double v[3], dist; };
constexpr int kSvRayCheck = 8;   // rays between two ballots

// keyframe::transformTo (keyframe.h:105-109): kfto.Pose.T() * (Pose * p + Pos - kfto.Pos); TooN's products are a dot product per row
// (of the transpose: per column), result = 0 and += in index order.
__device__ __forceinline__ void sv_transform_to(const double *H, const double *T, const double p[3], double o[3]) {
    double w[3];
    for (int i = 0; i < 3; i++) {
        double s = 0;
        s += H[3 * i] * p[0];
        s += H[3 * i + 1] * p[1];
        s += H[3 * i + 2] * p[2];
        w[i] = s + H[9 + i] - T[9 + i];
    }
    for (int i = 0; i < 3; i++) {
        double s = 0;
        s += T[i] * w[0];
        s += T[3 + i] * w[1];
        s += T[6 + i] * w[2];
        o[i] = s;
    }
}

__global__ __launch_bounds__(kSvThreads) void k_sv_ray_cross(SvStore st, SvGeom g, const int2 *pairs) {
    __shared__ SvRay rays[kSvThreads];
    __shared__ int wave_done[kSvThreads / 64];
    const int G = g.gw * g.gh, tid = threadIdx.x, wave = tid >> 6;
    const int t = pairs[blockIdx.x].x, h = pairs[blockIdx.x].y;
    const int c = blockIdx.y * kSvThreads + tid;
    const double *T = st.pose + (size_t)t * 13, *H = st.pose + (size_t)h * 13;
    const double *rho_h = st.rho + (size_t)h * G;
    uint8_t *vis = st.vis + (size_t)t * G;

    const double zero[3] = {0, 0, 0};
    double ro[3];
    sv_transform_to(H, T, zero, ro);                 // ray_orig (:89)

    // the target cell: point (:93), buble_size (:95, norm_size :79) and point - ray_orig
    double d[3] = {0, 0, 0}, bub = 0, lo = -1.0, hi = INFINITY;
    bool crossed = true;
    if (c < G) {
        const double r = st.rho[(size_t)t * G + c];
        double P[3];
        sv_cell_point(c % g.gw, c / g.gw, r, g, P);
        const double norm_size = sqrt((double)(g.bw * g.bw + g.bh * g.bh)) / g.zfm * T[12];   // util::norm(int, int)
        bub = norm_size / r;
        for (int i = 0; i < 3; i++) d[i] = P[i] * T[12] - ro[i];
        if (bub > 1e-140 && bub < 1e140) {
            const double b2 = bub * bub;
            lo = b2 * (1.0 - 1e-6);
            hi = b2 * (1.0 + 1e-6);
        }
        crossed = vis[c] == 0;
    }
    const bool hidden_before = crossed;

    bool done = __ballot(!crossed) == 0;
    for (int tile = 0; tile < G; tile += kSvThreads) {
        if ((tid & 63) == 0) wave_done[wave] = done;
        __syncthreads();                             // the last tile's reads are over; the flags are there
        bool all = true;
        for (int k = 0; k < kSvThreads / 64; k++) all = all && wave_done[k];
        if (all) break;
        const int hc = tile + tid;
        if (hc < G) {                                // the hidder's ray through cell hc: ray_pass (:90), ray_versor (:91), dist (depth_filler.cpp:175-177)
            double P[3], S[3], rp[3], u[3];
            sv_cell_point(hc % g.gw, hc / g.gw, rho_h[hc], g, P);
            for (int i = 0; i < 3; i++) S[i] = P[i] * H[12];
            sv_transform_to(H, T, S, rp);
            for (int i = 0; i < 3; i++) u[i] = rp[i] - ro[i];
            double nn = 0, pp = 0;
            for (int i = 0; i < 3; i++) nn += u[i] * u[i];
            const double inv = 1 / sqrt(nn);         // unit(v) = v * (1 / sqrt(v * v))
            for (int i = 0; i < 3; i++) rays[tid].v[i] = u[i] * inv;
            for (int i = 0; i < 3; i++) pp += P[i] * P[i];
            rays[tid].dist = sqrt(pp);               // norm(get3DPos(x, y) - Zeros): not scaled by K
        }
        __syncthreads();
        if (done) continue;
        const int n = min(kSvThreads, G - tile);
        for (int j0 = 0; j0 < n; j0 += kSvRayCheck) {
            const int j1 = min(j0 + kSvRayCheck, n);
            for (int j = j0; j < j1; j++) {
                const double vx = rays[j].v[0], vy = rays[j].v[1], vz = rays[j].v[2];
                const double cx = d[1] * vz - d[2] * vy, cy = d[2] * vx - d[0] * vz, cz = d[0] * vy - d[1] * vx;   // operator^
                double n2 = 0;
                n2 += cx * cx;
                n2 += cy * cy;
                n2 += cz * cz;
                if (!(n2 > hi)) {
                    if (n2 < lo || sqrt(n2) < bub) {
                        double along = 0;
                        along += d[0] * vx;
                        along += d[1] * vy;
                        along += d[2] * vz;
                        if (along > 0 && along < rays[j].dist) crossed = true;
                    }
                }
            }
            if (__ballot(!crossed) == 0) { done = true; break; }
        }
    }
    if (crossed && !hidden_before) vis[c] = 0;       // visibility = false (:109-110); nothing sets it back
}

struct SvPose { double m[13]; };
// a view's pose, and ResetVisibility (depth_filler.cpp:190-194) for its cells
__global__ __launch_bounds__(kSvThreads) void k_sv_set_view(double *pose, uint8_t *vis, int G, SvPose p) {
    const int c = blockIdx.x * kSvThreads + threadIdx.x;
    if (c < 13) pose[c] = p.m[c];
    if (c < G) vis[c] = 1;
}

}  // namespace edgehip

using namespace edgehip;

struct edgehip_ctx::SurfaceViews {
    edgehip_surface_views_params p;
    int gw, gh, bw, bh;
    size_t nvox;
    void *arena = nullptr;       // the view store
    double *rho, *s_rho, *pose, *part;
    uint8_t *vis;
    unsigned *plane = nullptr;   // [nz][ny][nx] voxel words
    int2 *pairs = nullptr;       // edgehip_surface_ray_cross's (target, hidder) list; grows on demand
    size_t pairs_cap = 0;
    SvMask stored;
};

void edgehip::surface_views_free(edgehip_ctx *c) {
    if (!c->sviews) return;
    (void)hipStreamSynchronize(c->stream);
    if (c->sviews->arena) (void)hipFree(c->sviews->arena);
    if (c->sviews->plane) (void)hipFree(c->sviews->plane);
    if (c->sviews->pairs) (void)hipFree(c->sviews->pairs);
    delete c->sviews;
    c->sviews = nullptr;
}

static SvGeom sv_geom(edgehip_ctx *c) {
    auto *v = c->sviews;
    SvGeom g;
    g.gw = v->gw; g.gh = v->gh; g.bw = v->bw; g.bh = v->bh;
    g.ppx = c->plan.ppx; g.ppy = c->plan.ppy; g.zfm = c->plan.zfm;
    return g;
}

static SvStore sv_store(edgehip_ctx *c) {
    auto *v = c->sviews;
    SvStore s;
    s.rho = v->rho; s.s_rho = v->s_rho; s.pose = v->pose; s.vis = v->vis;
    return s;
}

int edgehip_surface_views_enable(edgehip_ctx *c, const edgehip_surface_views_params *p) {
    EH_ENTER(c);
    if (!p) { surface_views_free(c); return 0; }
    int32_t gw, gh, bw, bh;
    if (depth_fill_geometry(c, &gw, &gh, &bw, &bh) != 0) {
        set_error("surface_views_enable: depth fill is not enabled (edgehip_depth_fill_enable)");
        return EDGEHIP_ERR_STATE;
    }
    if (p->capacity < 1 || p->capacity > kSvMaxViews || p->nx < 1 || p->ny < 1 || p->nz < 1) {
        set_error("surface_views_enable: capacity must be in [1, 1024] and every voxel dimension >= 1");
        return EDGEHIP_ERR_ARG;
    }
    surface_views_free(c);
    auto *v = new edgehip_ctx::SurfaceViews;
    v->p = *p;
    v->gw = gw; v->gh = gh; v->bw = bw; v->bh = bh;
    v->nvox = (size_t)p->nx * p->ny * p->nz;
    memset(&v->stored, 0, sizeof v->stored);
    const size_t cap = p->capacity, G = (size_t)gw * gh;
    const size_t bytes = 8 * cap * (2 * G + 13 + 6) + cap * G;
    auto fail = [&](const char *msg, int code) {
        (void)hipGetLastError();
        if (v->arena) (void)hipFree(v->arena);
        if (v->plane) (void)hipFree(v->plane);
        delete v;
        set_error(msg);
        return code;
    };
    if (hipMalloc(&v->arena, bytes) != hipSuccess) return fail("surface_views_enable: device allocation of the view store failed", EDGEHIP_ERR_MEMORY);
    if (hipMalloc((void **)&v->plane, 4 * v->nvox) != hipSuccess) return fail("surface_views_enable: device allocation of the voxel plane failed", EDGEHIP_ERR_MEMORY);
    char *q = (char *)v->arena;
    v->rho = (double *)q; q += 8 * cap * G;
    v->s_rho = (double *)q; q += 8 * cap * G;
    v->pose = (double *)q; q += 8 * cap * 13;
    v->part = (double *)q; q += 8 * cap * 6;
    v->vis = (uint8_t *)q;
    if (hipMemsetAsync(v->arena, 0, bytes, c->stream) != hipSuccess) return fail("surface_views_enable: hipMemsetAsync failed", EDGEHIP_ERR_DEVICE);
    c->sviews = v;
    return 0;
}

static int sv_check_view(edgehip_ctx *c, int view, const char *who) {
    if (!c->sviews) { set_error(std::string(who) + ": the view store is not enabled (edgehip_surface_views_enable)"); return EDGEHIP_ERR_STATE; }
    if (view < 0 || view >= c->sviews->p.capacity) { set_error(std::string(who) + ": view out of range"); return EDGEHIP_ERR_ARG; }
    return 0;
}

static int sv_set_view(edgehip_ctx *c, int view, const double *Pose, const double *Pos, double K) {
    auto *v = c->sviews;
    const int G = v->gw * v->gh;
    SvPose sp;
    memcpy(sp.m, Pose, 72);
    memcpy(sp.m + 9, Pos, 24);
    sp.m[12] = K;
    hipLaunchKernelGGL(k_sv_set_view, dim3((std::max(G, 13) + kSvThreads - 1) / kSvThreads), dim3(kSvThreads), 0, c->stream,
                       v->pose + (size_t)view * 13, v->vis + (size_t)view * G, G, sp);
    EH_LAUNCH_CHECK();
    v->stored.w[view >> 6] |= 1ull << (view & 63);
    return 0;
}

int edgehip_surface_view_capture(edgehip_ctx *c, int seq, int view, const double *Pose, const double *Pos, double K) {
    EH_ENTER(c);
    if (int e = sv_check_view(c, view, "surface_view_capture")) return e;
    if (seq < 0 || seq >= c->plan.nseq || !Pose || !Pos) { set_error("surface_view_capture: bad argument"); return EDGEHIP_ERR_ARG; }
    const double *rho, *s_rho;
    if (!depth_fill_grids(c, &rho, &s_rho)) { set_error("surface_view_capture: no edgehip_depth_fill since the fill was enabled"); return EDGEHIP_ERR_STATE; }
    auto *v = c->sviews;
    const size_t G = (size_t)v->gw * v->gh;
    EH_CHECK(hipMemcpyAsync(v->rho + view * G, rho + seq * G, 8 * G, hipMemcpyDeviceToDevice, c->stream));
    EH_CHECK(hipMemcpyAsync(v->s_rho + view * G, s_rho + seq * G, 8 * G, hipMemcpyDeviceToDevice, c->stream));
    return sv_set_view(c, view, Pose, Pos, K);
}

int edgehip_surface_view_upload(edgehip_ctx *c, int view, const double *rho, const double *s_rho, const double *Pose, const double *Pos, double K) {
    EH_ENTER(c);
    if (int e = sv_check_view(c, view, "surface_view_upload")) return e;
    if (!rho || !s_rho || !Pose || !Pos) { set_error("surface_view_upload: null argument"); return EDGEHIP_ERR_ARG; }
    auto *v = c->sviews;
    const size_t G = (size_t)v->gw * v->gh;
    EH_CHECK(hipMemcpyAsync(v->rho + view * G, rho, 8 * G, hipMemcpyHostToDevice, c->stream));
    EH_CHECK(hipMemcpyAsync(v->s_rho + view * G, s_rho, 8 * G, hipMemcpyHostToDevice, c->stream));
    if (int e = sv_set_view(c, view, Pose, Pos, K)) return e;
    EH_CHECK(hipStreamSynchronize(c->stream));   // the caller's arrays are free on return
    return 0;
}

int edgehip_surface_view_clear(edgehip_ctx *c, int view) {
    EH_ENTER(c);
    if (int e = sv_check_view(c, view, "surface_view_clear")) return e;
    c->sviews->stored.w[view >> 6] &= ~(1ull << (view & 63));
    return 0;
}

int edgehip_surface_space(edgehip_ctx *c, double *origin, double *size) {
    EH_ENTER(c);
    auto *v = c->sviews;
    if (!v) { set_error("surface_space: the view store is not enabled (edgehip_surface_views_enable)"); return EDGEHIP_ERR_STATE; }
    if (!origin || !size) { set_error("surface_space: null argument"); return EDGEHIP_ERR_ARG; }
    const int cap = v->p.capacity;
    hipLaunchKernelGGL(k_sv_bounds, dim3(cap), dim3(kSvThreads), 0, c->stream, sv_store(c), sv_geom(c), v->stored, v->part);
    EH_LAUNCH_CHECK();
    std::vector<double> part(6 * (size_t)cap);
    EH_CHECK(hipMemcpyAsync(part.data(), v->part, 48 * (size_t)cap, hipMemcpyDeviceToHost, c->stream));
    EH_CHECK(hipStreamSynchronize(c->stream));
    double mn[3] = {1e20, 1e20, 1e20}, mx[3] = {1e-20, 1e-20, 1e-20};
    for (int k = 0; k < cap; k++) {
        if (!v->stored.has(k)) continue;
        for (int i = 0; i < 3; i++) {
            if (part[6 * k + i] < mn[i]) mn[i] = part[6 * k + i];
            if (part[6 * k + 3 + i] > mx[i]) mx[i] = part[6 * k + 3 + i];
        }
    }
    for (int i = 0; i < 3; i++) { origin[i] = mn[i]; size[i] = mx[i] - mn[i]; }
    return 0;
}

int edgehip_surface_integrate(edgehip_ctx *c, const double *origin, const double *size, int n_cast, const int32_t *cast_views, int accumulate) {
    EH_ENTER(c);
    auto *v = c->sviews;
    if (!v) { set_error("surface_integrate: the view store is not enabled (edgehip_surface_views_enable)"); return EDGEHIP_ERR_STATE; }
    if (!origin || !size || (cast_views && n_cast < 0)) { set_error("surface_integrate: bad argument"); return EDGEHIP_ERR_ARG; }
    SvBox b;
    const int n[3] = {v->p.nx, v->p.ny, v->p.nz};
    for (int i = 0; i < 3; i++) {
        if (!(origin[i] == origin[i]) || std::isinf(origin[i]) || !(size[i] > 0.0) || std::isinf(size[i])) {
            set_error("surface_integrate: the box needs a finite origin and a finite, positive size");
            return EDGEHIP_ERR_ARG;
        }
        b.origin[i] = origin[i];
        b.n[i] = (unsigned)n[i];
        b.block[i] = size[i] / (double)b.n[i];   // OcGrid's block_size (:123)
    }
    b.min_block = b.block[0];                    // TooN::min_value
    for (int i = 1; i < 3; i++)
        if (b.block[i] < b.min_block) b.min_block = b.block[i];
    SvMask cast;
    if (!cast_views) {
        cast = v->stored;
    } else {
        memset(&cast, 0, sizeof cast);
        for (int j = 0; j < n_cast; j++) {
            const int k = cast_views[j];
            if (k < 0 || k >= v->p.capacity) { set_error("surface_integrate: casting view out of range"); return EDGEHIP_ERR_ARG; }
            if (v->stored.has(k)) cast.w[k >> 6] |= 1ull << (k & 63);   // rayCutSurface returns at once for a key frame without a grid (:237)
        }
    }
    const int G = v->gw * v->gh, cap = v->p.capacity;
    const size_t n16 = v->nvox / 4;
    const int nblk = (int)std::min<size_t>((n16 + kSvThreads - 1) / kSvThreads + 1, 256 * 64);
    hipLaunchKernelGGL(k_sv_clear, dim3(nblk), dim3(kSvThreads), 0, c->stream, (uint4 *)v->plane, n16, v->plane + 4 * n16, (int)(v->nvox - 4 * n16));
    EH_LAUNCH_CHECK();
    const dim3 grid((G + kSvThreads - 1) / kSvThreads, cap);
    hipLaunchKernelGGL(k_sv_rays, grid, dim3(kSvThreads), 0, c->stream, sv_store(c), sv_geom(c), b, cast, v->plane);
    EH_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sv_test, grid, dim3(kSvThreads), 0, c->stream, sv_store(c), sv_geom(c), b, v->stored, (const unsigned *)v->plane, accumulate);
    EH_LAUNCH_CHECK();
    return 0;
}

int edgehip_surface_ray_cross(edgehip_ctx *c, int n_pairs, const int32_t *targets, const int32_t *hidders, int accumulate) {
    EH_ENTER(c);
    auto *v = c->sviews;
    if (!v) { set_error("surface_ray_cross: the view store is not enabled (edgehip_surface_views_enable)"); return EDGEHIP_ERR_STATE; }
    const bool every = !targets && !hidders && n_pairs < 0;
    if (!every && (n_pairs < 0 || (n_pairs > 0 && (!targets || !hidders)))) {
        set_error("surface_ray_cross: n_pairs >= 0 needs both lists; both NULL with n_pairs < 0 means every ordered pair");
        return EDGEHIP_ERR_ARG;
    }
    const int cap = v->p.capacity;
    std::vector<int2> list;
    if (every) {
        for (int t = 0; t < cap; t++)
            for (int h = 0; h < cap; h++)
                if (t != h && v->stored.has(t) && v->stored.has(h)) list.push_back(make_int2(t, h));
    } else {
        for (int j = 0; j < n_pairs; j++) {
            const int t = targets[j], h = hidders[j];
            if (t < 0 || t >= cap || h < 0 || h >= cap) { set_error("surface_ray_cross: view out of range"); return EDGEHIP_ERR_ARG; }
            if (t == h) { set_error("surface_ray_cross: a pair needs two different views"); return EDGEHIP_ERR_ARG; }
        }
        for (int j = 0; j < n_pairs; j++)   // checkDFRayCrossExaustive returns at once when either key frame has no grid (:73)
            if (v->stored.has(targets[j]) && v->stored.has(hidders[j])) list.push_back(make_int2(targets[j], hidders[j]));
    }
    const size_t G = (size_t)v->gw * v->gh;
    if (!accumulate) EH_CHECK(hipMemsetAsync(v->vis, 1, (size_t)cap * G, c->stream));   // ResetVisibility
    if (list.empty()) return 0;
    if (list.size() > v->pairs_cap) {
        if (v->pairs) EH_CHECK(hipFree(v->pairs));   // waits for the launches that read it
        v->pairs = nullptr;
        v->pairs_cap = 0;
        if (hipMalloc((void **)&v->pairs, list.size() * sizeof(int2)) != hipSuccess) {
            (void)hipGetLastError();
            set_error("surface_ray_cross: device allocation of the pair list failed");
            return EDGEHIP_ERR_MEMORY;
        }
        v->pairs_cap = list.size();
    }
    EH_CHECK(hipMemcpyAsync(v->pairs, list.data(), list.size() * sizeof(int2), hipMemcpyHostToDevice, c->stream));   // pageable: staged on return
    hipLaunchKernelGGL(k_sv_ray_cross, dim3((unsigned)list.size(), (unsigned)((G + kSvThreads - 1) / kSvThreads)), dim3(kSvThreads), 0, c->stream,
                       sv_store(c), sv_geom(c), (const int2 *)v->pairs);
    EH_LAUNCH_CHECK();
    return 0;
}

int edgehip_download_surface_visibilities_batch(edgehip_ctx *c, int n, const int32_t *views, uint8_t *const *vis) {
    EH_ENTER(c);
    auto *v = c->sviews;
    if (!v) { set_error("download_surface_visibility: the view store is not enabled (edgehip_surface_views_enable)"); return EDGEHIP_ERR_STATE; }
    if (n < 1 || !views || !vis) { set_error("download_surface_visibility: bad argument"); return EDGEHIP_ERR_ARG; }
    for (int j = 0; j < n; j++) {
        if (views[j] < 0 || views[j] >= v->p.capacity) { set_error("download_surface_visibility: view out of range"); return EDGEHIP_ERR_ARG; }
        if (!v->stored.has(views[j])) { set_error("download_surface_visibility: the view holds no grid"); return EDGEHIP_ERR_STATE; }
    }
    const size_t G = (size_t)v->gw * v->gh;
    for (int j = 0; j < n; j++)
        if (vis[j]) EH_CHECK(hipMemcpyAsync(vis[j], v->vis + views[j] * G, G, hipMemcpyDeviceToHost, c->stream));
    EH_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int edgehip_download_surface_visibility(edgehip_ctx *c, int view, uint8_t *vis) {
    return edgehip_download_surface_visibilities_batch(c, 1, &view, &vis);
}
