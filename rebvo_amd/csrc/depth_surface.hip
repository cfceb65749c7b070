// depth_surface.hip — what REBVO's callers take from a depth_filler grid (src/visualizer/depth_filler.cpp, depth_filler.h), for every
// sequence of a context, from the grids of the last edgehip_depth_fill (depth_fill.hip):
//   k_depth_surface  per cell: get3DPos (depth_filler.h:115-122), computeDistance(Zeros)'s dist and current_min_dist (:170-180),
//                    calcSurfNormals (:358-373) and calcSurfArea (:377-389).  One workgroup per sequence; a lane recomputes the
//                    points of its neighbours instead of exchanging them; the minimum distance is an LDS reduction (exact: dist >= 0
//                    and keep_min never takes a NaN, so the order does not matter).
//   k_depth_image    per pixel: getImgRho (depth_filler.h:246-280) or getImgRhoTriInterp (:203-244) with s_rho, at every integer pixel.
//                    A store stream: one workgroup per (row band, sequence); the band's column terms (xf, xc, dx) are formed once per
//                    pixel column and its grid rows converted to float once, both into LDS; each lane then writes 4 pixels of a row
//                    of both planes with 16-B nontemporal stores (nothing on the GPU reads the image back).
// The reference's types are followed exactly: get3DPos rounds the shifted cell centre to float and subtracts the principal point in
// float, then divides by the double zfm and by rho in double; both interpolations compute entirely in float, so the fp32 planes
// hold the reference's double results exactly.  '/' and sqrt are the compiler's correctly rounded operations, and -ffp-contract=off
// keeps every product and sum separately rounded.
#include "ctx.h"

#include <cmath>
#include <cstring>

namespace edgehip {

constexpr int kDsThreads = 256;
constexpr int kDiThreads = 256;
constexpr int kDiBandRows = 16;             // pixel rows per image workgroup: 30 bands x 1024 sequences at 752x480
constexpr size_t kDiLdsMax = 48 * 1024;     // LDS of an image workgroup: column terms + the band's grid rows as float

typedef float f4 __attribute__((ext_vector_type(4)));

struct DsArgs {
    const double *rho;         // [nseq][G] the fill's grids
    double *point, *normal;    // [nseq][G][3]
    float *area;               // [nseq][G]
    double *dist;              // [nseq][G]
    double *min_dist;          // [nseq]
    int gw, gh, bw, bh;
    float ppx, ppy;
    double zfm;
};

// get3DPos(x, y) (depth_filler.h:115-122): Img2Hom<float> of the cell centre ((float)x + 0.5) * bw — a double product rounded to
// float — minus the principal point in float; x / zfm in double (cam_model::zfm is a double); TooN's Vector / rho element-wise.
__device__ __forceinline__ void ds_point(const double *rho, int x, int y, const DsArgs &a, double P[3]) {
    const float ix = (float)(((double)(float)x + 0.5) * (double)a.bw);
    const float iy = (float)(((double)(float)y + 0.5) * (double)a.bh);
    const float hx = ix - a.ppx, hy = iy - a.ppy;
    const double r = rho[y * a.gw + x];
    P[0] = ((double)hx / a.zfm) / r;
    P[1] = ((double)hy / a.zfm) / r;
    P[2] = 1.0 / r;
}

__device__ __forceinline__ double ds_dot(const double u[3], const double v[3]) {   // TooN operator*: result = 0, += in index order
    double s = 0;
    s += u[0] * v[0];
    s += u[1] * v[1];
    s += u[2] * v[2];
    return s;
}

__device__ __forceinline__ void ds_cross(const double u[3], const double v[3], double o[3]) {   // TooN operator^
    o[0] = u[1] * v[2] - u[2] * v[1];
    o[1] = u[2] * v[0] - u[0] * v[2];
    o[2] = u[0] * v[1] - u[1] * v[0];
}

__global__ __launch_bounds__(kDsThreads) void k_depth_surface(DsArgs a) {
    __shared__ double part[kDsThreads];
    const int seq = blockIdx.x, tid = threadIdx.x;
    const int gw = a.gw, gh = a.gh, G = gw * gh;
    const double *rho = a.rho + (size_t)seq * G;
    double *point = a.point + (size_t)seq * G * 3, *normal = a.normal + (size_t)seq * G * 3, *dist = a.dist + (size_t)seq * G;
    float *area = a.area + (size_t)seq * G;
    const double qnan = __builtin_nan("");
    double mn = 1e20;   // current_min_dist's start
    for (int c = tid; c < G; c += kDsThreads) {
        const int x = c % gw, y = c / gw;
        double P[3];
        ds_point(rho, x, y, a, P);
        point[3 * c] = P[0]; point[3 * c + 1] = P[1]; point[3 * c + 2] = P[2];
        const double d = sqrt(ds_dot(P, P));   // TooN::norm(P - Zeros): subtracting +0 changes no value
        dist[c] = d;
        if (d < mn) mn = d;   // util::keep_min
        // calcSurfNormals' raster loop (x outer, y inner over [0, gw-2] x [0, gh-2]) writes (x, y) and then (x+1, y+1): the last
        // write of a cell is its own step where it has one, else the step of (x-1, y-1); (gw-1, 0), (0, gh-1) and every cell of a
        // 1-wide grid are never written (NaN here: uninitialised in the reference).  calcSurfArea writes (x, y) only.
        const bool own = x <= gw - 2 && y <= gh - 2;
        const int ox = own ? x : x - 1, oy = own ? y : y - 1;
        double n[3] = {qnan, qnan, qnan};
        float ar = __builtin_nanf("");
        if (ox >= 0 && oy >= 0 && ox <= gw - 2 && oy <= gh - 2) {
            double P00[3], P01[3], P10[3], P11[3];
            ds_point(rho, ox, oy, a, P00);
            ds_point(rho, ox + 1, oy, a, P01);
            ds_point(rho, ox, oy + 1, a, P10);
            ds_point(rho, ox + 1, oy + 1, a, P11);
            double e1[3], e2[3], f1[3], f2[3], u[3], v[3];
            for (int i = 0; i < 3; i++) {
                e1[i] = P01[i] - P00[i];
                e2[i] = P10[i] - P00[i];
                f1[i] = P01[i] - P11[i];
                f2[i] = P10[i] - P11[i];
            }
            ds_cross(e1, e2, u);
            ds_cross(f1, f2, v);
            const double uu = ds_dot(u, u), vv = ds_dot(v, v);
            const double su = 1 / sqrt(uu), sv = 1 / sqrt(vv);   // TooN::unit(v) = v * (1 / sqrt(v * v))
            for (int i = 0; i < 3; i++) n[i] = (-(u[i] * su) + v[i] * sv) / 2;
            if (own) ar = (float)((sqrt(uu) + sqrt(vv)) / 2);   // df_point::area is a float
        }
        normal[3 * c] = n[0]; normal[3 * c + 1] = n[1]; normal[3 * c + 2] = n[2];
        area[c] = ar;
    }
    part[tid] = mn;
    __syncthreads();
    for (int s = kDsThreads / 2; s > 0; s >>= 1) {
        if (tid < s && part[tid + s] < part[tid]) part[tid] = part[tid + s];
        __syncthreads();
    }
    if (tid == 0) a.min_dist[seq] = part[0];
}

struct DiArgs {
    const double *rho, *s_rho;   // [nseq][G]
    float *out_rho, *out_srho;   // [nseq][h][w]
    int w, h, gw, gh, bw, bh, mode, nrows;   // nrows: grid rows of LDS per workgroup
};

// getImgRho's / getImgRhoTriInterp's index terms of one coordinate: float x_histo = x / (float)bw - 0.5 (a float division, then a
// double subtraction rounded back to float); f / c = floor / ceil clamped to [0, n-1] (std::max(float, double) and std::min in
// double, then int); d = x_histo - f in float.  At x = 0, ceil(-0.5) = -0 gives f = c = 0 and d = -0.5 (the formula extrapolates).
__device__ __forceinline__ void di_terms(int x, int b, int n, int &f, int &c, float &d) {
    const float xh = (float)((double)((float)x / (float)b) - 0.5);
    const float fl = floorf(xh), ce = ceilf(xh);
    f = fl < 0.0f ? 0 : (fl > (float)(n - 1) ? n - 1 : (int)fl);
    c = ce < 0.0f ? 0 : (ce > (float)(n - 1) ? n - 1 : (int)ce);
    d = xh - (float)f;
}

__device__ __forceinline__ void di_pixel(int mode, float dx, float dy, float r00, float r10, float r01, float r11, float s00, float s10,
                                         float s01, float s11, float &r, float &s) {
    if (mode == EDGEHIP_DEPTH_IMAGE_BILINEAR) {   // depth_filler.h:269, 277
        r = r00 * (1 - dx) * (1 - dy) + r10 * dx * (1 - dy) + r01 * (1 - dx) * dy + r11 * dx * dy;
        s = s00 * (1 - dx) * (1 - dy) + s10 * dx * (1 - dy) + s01 * (1 - dx) * dy + s11 * dx * dy;
    } else if (dx > dy) {                         // depth_filler.h:223-239, s_rho as written (srho10 - srho11)
        r = r00 + dx * (r10 - r00) + dy * (r11 - r10);
        s = s00 + dx * (s10 - s11) + dy * (s11 - s10);
    } else {
        r = r00 + dy * (r01 - r00) + dx * (r11 - r01);
        s = s00 + dy * (s01 - s11) + dx * (s11 - s01);
    }
}

__global__ __launch_bounds__(kDiThreads) void k_depth_image(DiArgs a) {
    extern __shared__ __align__(16) unsigned char di_lds[];
    const int seq = blockIdx.y, tid = threadIdx.x;
    const int w = a.w, gw = a.gw, G = gw * a.gh;
    const int r0 = blockIdx.x * kDiBandRows, r1 = min(a.h, r0 + kDiBandRows);
    int *cf = (int *)di_lds, *cc = cf + w;
    float *cd = (float *)(cc + w);
    float *gr = cd + w, *gs = gr + (size_t)a.nrows * gw;   // grid rows g0 .. g0 + nrows - 1 as float
    int g0, g1, t0;
    float td;
    di_terms(r0, a.bh, a.gh, g0, t0, td);
    di_terms(r1 - 1, a.bh, a.gh, t0, g1, td);
    const int ng = min(g1 - g0 + 1, a.nrows);   // g1 - g0 + 1 <= nrows (edgehip_depth_surface_enable sizes it); f, c are monotone in the row
    for (int x = tid; x < w; x += kDiThreads) di_terms(x, a.bw, gw, cf[x], cc[x], cd[x]);
    const double *rho = a.rho + (size_t)seq * G, *srho = a.s_rho + (size_t)seq * G;
    for (int i = tid; i < ng * gw; i += kDiThreads) {
        gr[i] = (float)rho[(size_t)g0 * gw + i];
        gs[i] = (float)srho[(size_t)g0 * gw + i];
    }
    __syncthreads();
    float *orho = a.out_rho + (size_t)seq * w * a.h, *osrho = a.out_srho + (size_t)seq * w * a.h;
    const int nq = (w + 3) / 4;   // 4-pixel groups per row
    const bool vec = (w & 3) == 0;
    for (int item = tid; item < (r1 - r0) * nq; item += kDiThreads) {
        const int py = r0 + item / nq, x0 = (item % nq) * 4;
        int yf, yc;
        float dy;
        di_terms(py, a.bh, a.gh, yf, yc, dy);
        const float *rf = gr + (yf - g0) * gw, *rc = gr + (yc - g0) * gw, *sf = gs + (yf - g0) * gw, *sc = gs + (yc - g0) * gw;
        float r[4], s[4];
        for (int j = 0; j < 4; j++) {
            const int x = min(x0 + j, w - 1);
            const int xf = cf[x], xc = cc[x];
            di_pixel(a.mode, cd[x], dy, rf[xf], rf[xc], rc[xf], rc[xc], sf[xf], sf[xc], sc[xf], sc[xc], r[j], s[j]);
        }
        const size_t o = (size_t)py * w + x0;
        if (vec) {
            __builtin_nontemporal_store((f4){r[0], r[1], r[2], r[3]}, (f4 *)(orho + o));
            __builtin_nontemporal_store((f4){s[0], s[1], s[2], s[3]}, (f4 *)(osrho + o));
        } else {
            for (int j = 0; j < 4 && x0 + j < w; j++) {
                __builtin_nontemporal_store(r[j], orho + o + j);
                __builtin_nontemporal_store(s[j], osrho + o + j);
            }
        }
    }
}

}  // namespace edgehip

using namespace edgehip;

struct edgehip_ctx::DepthSurface {
    edgehip_depth_surface_params p;
    int gw, gh, bw, bh;
    int nrows;                 // grid rows an image band needs at most
    void *arena = nullptr;     // per-cell products (p.surface)
    double *point, *normal, *dist, *min_dist;
    float *area;
    float *img = nullptr;      // [2][nseq][h][w] rho then s_rho planes (p.image_mode)
};

void edgehip::depth_surface_free(edgehip_ctx *c) {
    if (!c->dsurf) return;
    (void)hipStreamSynchronize(c->stream);
    if (c->dsurf->arena) (void)hipFree(c->dsurf->arena);
    if (c->dsurf->img) (void)hipFree(c->dsurf->img);
    delete c->dsurf;
    c->dsurf = nullptr;
}

int edgehip_depth_surface_enable(edgehip_ctx *c, const edgehip_depth_surface_params *p) {
    EH_ENTER(c);
    if (!p) { depth_surface_free(c); return 0; }
    if (p->image_mode < EDGEHIP_DEPTH_IMAGE_OFF || p->image_mode > EDGEHIP_DEPTH_IMAGE_TRIANGLE) {
        set_error("depth_surface_enable: image_mode must be one of EDGEHIP_DEPTH_IMAGE_*");
        return EDGEHIP_ERR_ARG;
    }
    int32_t gw, gh, bw, bh;
    if (depth_fill_geometry(c, &gw, &gh, &bw, &bh) != 0) {
        set_error("depth_surface_enable: depth fill is not enabled (edgehip_depth_fill_enable)");
        return EDGEHIP_ERR_STATE;
    }
    depth_surface_free(c);
    if (!p->surface && !p->image_mode) return 0;
    const int nrows = (kDiBandRows - 1) / bh + 3;
    const size_t lds = 12 * (size_t)c->plan.w + 8 * (size_t)nrows * gw;
    if (p->image_mode && lds > kDiLdsMax) {
        set_error("depth_surface_enable: the image's band does not fit in LDS (grid too wide)");
        return EDGEHIP_ERR_ARG;
    }
    auto *d = new edgehip_ctx::DepthSurface;
    d->p = *p;
    d->gw = gw; d->gh = gh; d->bw = bw; d->bh = bh;
    d->nrows = nrows;
    const size_t B = c->plan.nseq, G = (size_t)gw * gh;
    auto fail = [&](const char *msg, int code) {
        (void)hipGetLastError();
        if (d->arena) (void)hipFree(d->arena);
        if (d->img) (void)hipFree(d->img);
        delete d;
        set_error(msg);
        return code;
    };
    if (p->surface) {
        const size_t bytes = 8 * B * (7 * G + 1) + 4 * B * G;
        if (hipMalloc(&d->arena, bytes) != hipSuccess) return fail("depth_surface_enable: device allocation failed", EDGEHIP_ERR_MEMORY);
        char *q = (char *)d->arena;
        d->point = (double *)q; q += 8 * B * G * 3;
        d->normal = (double *)q; q += 8 * B * G * 3;
        d->dist = (double *)q; q += 8 * B * G;
        d->min_dist = (double *)q; q += 8 * B;
        d->area = (float *)q;
        // NaN until the first edgehip_depth_surface
        if (hipMemsetAsync(d->arena, 0xFF, bytes, c->stream) != hipSuccess) return fail("depth_surface_enable: hipMemsetAsync failed", EDGEHIP_ERR_DEVICE);
    }
    if (p->image_mode) {
        const size_t bytes = 8 * B * (size_t)c->plan.w * c->plan.h;
        if (hipMalloc(&d->img, bytes) != hipSuccess) return fail("depth_surface_enable: device allocation of the depth image failed", EDGEHIP_ERR_MEMORY);
        if (hipMemsetAsync(d->img, 0xFF, bytes, c->stream) != hipSuccess) return fail("depth_surface_enable: hipMemsetAsync failed", EDGEHIP_ERR_DEVICE);
    }
    c->dsurf = d;
    return 0;
}

int edgehip_depth_surface(edgehip_ctx *c) {
    EH_ENTER(c);
    auto *d = c->dsurf;
    if (!d) { set_error("depth_surface: depth surface is not enabled (edgehip_depth_surface_enable)"); return EDGEHIP_ERR_STATE; }
    const double *rho, *s_rho;
    if (!depth_fill_grids(c, &rho, &s_rho)) { set_error("depth_surface: no edgehip_depth_fill since the fill was enabled"); return EDGEHIP_ERR_STATE; }
    const int B = c->plan.nseq;
    if (d->p.surface) {
        DsArgs a;
        a.rho = rho;
        a.point = d->point; a.normal = d->normal; a.area = d->area; a.dist = d->dist; a.min_dist = d->min_dist;
        a.gw = d->gw; a.gh = d->gh; a.bw = d->bw; a.bh = d->bh;
        a.ppx = c->plan.ppx; a.ppy = c->plan.ppy; a.zfm = c->plan.zfm;
        hipLaunchKernelGGL(k_depth_surface, dim3(B), dim3(kDsThreads), 0, c->stream, a);
        EH_LAUNCH_CHECK();
    }
    if (d->p.image_mode) {
        DiArgs a;
        a.rho = rho; a.s_rho = s_rho;
        const size_t plane = (size_t)B * c->plan.w * c->plan.h;
        a.out_rho = d->img; a.out_srho = d->img + plane;
        a.w = c->plan.w; a.h = c->plan.h; a.gw = d->gw; a.gh = d->gh; a.bw = d->bw; a.bh = d->bh;
        a.mode = d->p.image_mode; a.nrows = d->nrows;
        const size_t lds = 12 * (size_t)a.w + 8 * (size_t)d->nrows * d->gw;
        hipLaunchKernelGGL(k_depth_image, dim3((a.h + kDiBandRows - 1) / kDiBandRows, B), dim3(kDiThreads), lds, c->stream, a);
        EH_LAUNCH_CHECK();
    }
    return 0;
}

int edgehip_download_depth_surfaces_batch(edgehip_ctx *c, int n, const int32_t *seqs, double *const *point, double *const *normal,
                                          float *const *area, double *const *dist, double *const *min_dist) {
    EH_ENTER(c);
    auto *d = c->dsurf;
    if (!d || !d->p.surface) { set_error("download_depth_surface: the per-cell surface is not enabled"); return EDGEHIP_ERR_STATE; }
    if (n < 1 || !seqs) { set_error("download_depth_surface: bad argument"); return EDGEHIP_ERR_ARG; }
    for (int j = 0; j < n; j++)
        if (seqs[j] < 0 || seqs[j] >= c->plan.nseq) { set_error("download_depth_surface: sequence out of range"); return EDGEHIP_ERR_ARG; }
    const size_t G = (size_t)d->gw * d->gh;
    for (int j = 0; j < n; j++) {
        const size_t o = (size_t)seqs[j] * G;
        if (point && point[j]) EH_CHECK(hipMemcpyAsync(point[j], d->point + 3 * o, 24 * G, hipMemcpyDeviceToHost, c->stream));
        if (normal && normal[j]) EH_CHECK(hipMemcpyAsync(normal[j], d->normal + 3 * o, 24 * G, hipMemcpyDeviceToHost, c->stream));
        if (area && area[j]) EH_CHECK(hipMemcpyAsync(area[j], d->area + o, 4 * G, hipMemcpyDeviceToHost, c->stream));
        if (dist && dist[j]) EH_CHECK(hipMemcpyAsync(dist[j], d->dist + o, 8 * G, hipMemcpyDeviceToHost, c->stream));
        if (min_dist && min_dist[j]) EH_CHECK(hipMemcpyAsync(min_dist[j], d->min_dist + seqs[j], 8, hipMemcpyDeviceToHost, c->stream));
    }
    EH_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int edgehip_download_depth_surface(edgehip_ctx *c, int seq, double *point, double *normal, float *area, double *dist, double *min_dist) {
    return edgehip_download_depth_surfaces_batch(c, 1, &seq, &point, &normal, &area, &dist, &min_dist);
}

int edgehip_download_depth_images_batch(edgehip_ctx *c, int n, const int32_t *seqs, float *const *rho, float *const *s_rho) {
    EH_ENTER(c);
    auto *d = c->dsurf;
    if (!d || !d->p.image_mode) { set_error("download_depth_image: the depth image is not enabled"); return EDGEHIP_ERR_STATE; }
    if (n < 1 || !seqs) { set_error("download_depth_image: bad argument"); return EDGEHIP_ERR_ARG; }
    for (int j = 0; j < n; j++)
        if (seqs[j] < 0 || seqs[j] >= c->plan.nseq) { set_error("download_depth_image: sequence out of range"); return EDGEHIP_ERR_ARG; }
    const size_t N = (size_t)c->plan.w * c->plan.h, plane = N * c->plan.nseq;
    for (int j = 0; j < n; j++) {
        const size_t o = (size_t)seqs[j] * N;
        if (rho && rho[j]) EH_CHECK(hipMemcpyAsync(rho[j], d->img + o, 4 * N, hipMemcpyDeviceToHost, c->stream));
        if (s_rho && s_rho[j]) EH_CHECK(hipMemcpyAsync(s_rho[j], d->img + plane + o, 4 * N, hipMemcpyDeviceToHost, c->stream));
    }
    EH_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int edgehip_download_depth_image(edgehip_ctx *c, int seq, float *rho, float *s_rho) {
    return edgehip_download_depth_images_batch(c, 1, &seq, &rho, &s_rho);
}

int edgehip_depth_image_device(edgehip_ctx *c, int first, int count, float *rho_dev, float *s_rho_dev) {
    EH_ENTER(c);
    auto *d = c->dsurf;
    if (!d || !d->p.image_mode) { set_error("depth_image_device: the depth image is not enabled"); return EDGEHIP_ERR_STATE; }
    if (first < 0 || count < 1 || first + count > c->plan.nseq) { set_error("depth_image_device: sequence range out of bounds"); return EDGEHIP_ERR_ARG; }
    const size_t N = (size_t)c->plan.w * c->plan.h, plane = N * c->plan.nseq;
    if (rho_dev) EH_CHECK(hipMemcpyAsync(rho_dev, d->img + first * N, 4 * N * count, hipMemcpyDeviceToDevice, c->stream));
    if (s_rho_dev) EH_CHECK(hipMemcpyAsync(s_rho_dev, d->img + plane + first * N, 4 * N * count, hipMemcpyDeviceToDevice, c->stream));
    EH_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}
