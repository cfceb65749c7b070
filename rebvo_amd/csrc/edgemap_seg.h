// edgemap_seg.h — the receiving side of the reference's compressed edge map as rules local to one record, one segment or one step,
// stated once for the host (rebvo/edgemap_com.h: decode, hide_visible, fill_depth_map) and the device (edgemap_decode.hip,
// depth_fill.hip).  From edgemap_com::getPair (src/CommLib/edgemap_com.cpp:46-86), edgemap_com::TransformPos (:106-127),
// edgemap_com_decoder::HideVisible (:443-473) and edgemap_com_decoder::fillDepthMap (:475-528), in their types: what is float there is
// float here, what is double there is double here, and every product and sum is rounded on its own (-ffp-contract=off).
//
// getPair is a cursor walk, but which records start a segment is local.  The cursor stands on record i at the top of a call iff no
// earlier call consumed it; a call consumes its k0 and, when its k1 closes a polyline (rho < 0), that k1 too.  So record i starts a
// segment iff  i < kl_num - 1,  rho[i] != 0,  and not (rho[i] < 0 and i >= 1 and rho[i - 1] > 0)  — a negative record behind a
// positive one was that one's closing k1 — and its partner is record i again when rho[i] < 0 or rho[i + 1] == 0, else record i + 1.
// (tests/test_edgemap_decode_cpu.py enumerates every sign pattern up to length 10 against the walk.)
// Domain: the walk reads "closes a polyline" from the float kl1.rho < 0 after the division, the rule from the integer rho.  The two
// agree while COMPRESSED_RHO_SCALING / rho_scale is a finite positive float, i.e. for rho_scale > 0, finite, above about 5e-36; below
// that the quotient is inf, every rho is +-0 and the walk emits segments the rule does not.  edgehip_upload_edgemap refuses such a
// rho_scale; edgehip_edgemap_compress stores the scale it is given unchecked, as it always took any double.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define REBVO_SEG_HD __host__ __device__ inline
#else
#define REBVO_SEG_HD inline
#endif

namespace rebvo {
namespace edgemap {

struct SegPoint { float x, y, rho, s_rho; };   // uncompressed_kl (PPoint3D<float>)
struct SegCam {                                // what the decoder reads of cam_model
    float ppx, ppy;
    double zfm;
    uint32_t w, h;                             // cam.sz (u_int)
};

constexpr float kSegRhoScaling = (float)(32767.0 / 20);   // COMPRESSED_RHO_SCALING
constexpr float kSegSRhoScaling = (float)(255.0 / 20);    // COMPRESSED_SRHO_SCALING
constexpr float kSegCRhoMin = (float)1e-3;                // CRHO_MIN, narrowed by the assignment to the float s_rho

REBVO_SEG_HD bool seg_starts(int rho_prev, int rho_i, int i, int kl_num) {   // rho_prev: rho[i - 1], anything for i == 0
    return i < kl_num - 1 && rho_i != 0 && !(rho_i < 0 && i >= 1 && rho_prev > 0);
}
REBVO_SEG_HD bool seg_partner_is_self(int rho_i, int rho_next) { return rho_i < 0 || rho_next == 0; }

// one record as getPair converts it; rho: abs(rho) for k0, the signed value for k1 (negated afterwards when negative)
REBVO_SEG_HD SegPoint seg_point(int x, int y, float rho, int s_rho, float rho_scale, double x_scaling, double y_scaling) {
    SegPoint o;
    o.rho = rho;
    o.rho /= kSegRhoScaling / rho_scale;
    o.x = (float)(x / x_scaling);
    o.y = (float)(y / y_scaling);
    o.s_rho = s_rho > 0 ? s_rho / kSegSRhoScaling : kSegCRhoMin;
    return o;
}
REBVO_SEG_HD void seg_pair(int x0, int y0, int rho0, int s0, int x1, int y1, int rho1, int s1, float rho_scale, double x_scaling,
                           double y_scaling, SegPoint *k0, SegPoint *k1) {
    *k0 = seg_point(x0, y0, (float)(rho0 < 0 ? -rho0 : rho0), s0, rho_scale, x_scaling, y_scaling);
    if (seg_partner_is_self(rho0, rho1)) { *k1 = *k0; return; }
    *k1 = seg_point(x1, y1, (float)rho1, s1, rho_scale, x_scaling, y_scaling);
    if (k1->rho < 0) k1->rho = -k1->rho;
}

// TransformPos: the point seen from the new view.  DPose row-major, k_em = em_pos.K, k_new = new_pos.K.
REBVO_SEG_HD SegPoint seg_transform_pos(const SegPoint &p, const double *DPose, const double *DPos, float k_em, float k_new, const SegCam &cam) {
    const float x = p.x - cam.ppx, y = p.y - cam.ppy;                      // Img2Hom<float>
    const double P0[3] = {(x / cam.zfm) / p.rho, (y / cam.zfm) / p.rho, 1.0 / p.rho};
    double P1[3];
    for (int r = 0; r < 3; r++) {
        double s = 0;
        for (int c = 0; c < 3; c++) s += DPose[3 * r + c] * P0[c];
        P1[r] = s * k_em + DPos[r];
    }
    SegPoint o;
    o.rho = (float)(1 / P1[2]);
    o.x = (float)(P1[0] * o.rho * cam.zfm);
    o.y = (float)(P1[1] * o.rho * cam.zfm);
    o.rho *= k_new;
    o.x = o.x + cam.ppx;                                                   // Hom2Img<float>
    o.y = o.y + cam.ppy;
    o.s_rho = p.s_rho * k_new;
    return o;
}
REBVO_SEG_HD bool seg_in_frame(const SegPoint &t, const SegCam &cam) {
    return t.x >= 0 && t.y >= 0 && t.x < (float)cam.w && t.y < (float)cam.h && t.rho > 0;
}
// HideVisible's test of one segment: true when the new view sees an end point
REBVO_SEG_HD bool seg_seen(const SegPoint &k0, const SegPoint &k1, const double *DPose, const double *DPos, float k_em, float k_new,
                           const SegCam &cam) {
    return seg_in_frame(seg_transform_pos(k0, DPose, DPos, k_em, k_new, cam), cam) ||
           seg_in_frame(seg_transform_pos(k1, DPose, DPos, k_em, k_new, cam), cam);
}

// cam_model::unprojectImgCordVec on the Vector<3, float> that makeVector(float, float, float) makes: float storage
REBVO_SEG_HD void seg_unproject(float x, float y, float rho, const SegCam &cam, double *out) {
    out[0] = (float)((double)((x - cam.ppx) / rho) / cam.zfm);
    out[1] = (float)((double)((y - cam.ppy) / rho) / cam.zfm);
    out[2] = (float)(1.0 / rho);
}
// fabs((p0 - p1) * p0) / norm(p0) / norm(p0 - p1), p1 unprojected with k0.rho as the reference writes it
REBVO_SEG_HD double seg_cangle(const SegPoint &k0, const SegPoint &k1, const SegCam &cam) {
    double p0[3], p1[3], d[3];
    seg_unproject(k0.x, k0.y, k0.rho, cam, p0);
    seg_unproject(k1.x, k1.y, k0.rho, cam, p1);
    for (int i = 0; i < 3; i++) d[i] = p0[i] - p1[i];
    double dp = 0, n0 = 0, nd = 0;
    for (int i = 0; i < 3; i++) dp += d[i] * p0[i];
    for (int i = 0; i < 3; i++) n0 += p0[i] * p0[i];
    for (int i = 0; i < 3; i++) nd += d[i] * d[i];
    return fabs(dp) / sqrt(n0) / sqrt(nd);
}

// one segment's walk over the grid: the direction, its length and the per-step constants of fillDepthMap (:498-509)
struct SegSteps {
    int n;                 // steps: the i = 0, 1, ... with i < nt; 0 when a gate skips the segment or it is degenerate
    double q0x, q0y, tx, ty, r1, rho0, kl_I;
};
enum SegGate { kSegFolded = 0, kSegGateSigma = 1, kSegGateSum = 2, kSegGateRel = 3, kSegGateAngle = 4, kSegDegenerate = 5 };

// cos_a: cos(a_thresh * M_PI / 180.0), taken once by the caller.  *gate (may be null): which test ended the segment.
REBVO_SEG_HD SegSteps seg_steps(const SegPoint &k0, const SegPoint &k1, const SegCam &cam, double v_thresh, double cos_a, int *gate) {
    SegSteps s;
    s.n = 0;
    s.q0x = s.q0y = s.tx = s.ty = s.r1 = s.rho0 = s.kl_I = 0;
    int g = kSegFolded;
    if (k0.s_rho * kSegSRhoScaling > 254.0 || k1.s_rho * kSegSRhoScaling > 254.0) g = kSegGateSigma;
    else if (k0.s_rho + k1.s_rho > k0.rho + k1.rho) g = kSegGateSum;
    else if (k0.rho / k0.s_rho < v_thresh || k1.rho / k1.s_rho < v_thresh) g = kSegGateRel;
    else if (seg_cangle(k0, k1, cam) > cos_a) g = kSegGateAngle;           // (a NaN cangle does not skip)
    if (g == kSegFolded) {
        const double dx = k1.x - k0.x, dy = k1.y - k0.y;                   // float differences
        const double nt = sqrt(dx * dx + dy * dy);
        s.q0x = k0.x; s.q0y = k0.y;
        s.tx = dx / nt; s.ty = dy / nt;
        s.r1 = (k1.rho - k0.rho) / nt;
        s.rho0 = k0.rho;
        const double sr = (k0.s_rho + k1.s_rho) / 2;
        s.kl_I = 1 / (sr * sr);
        // for (int i = 0; i < nt; i++): i < nt compares in double; nt <= 361 for byte coordinates, bounded here for any scaling
        if (!(nt > 0)) g = kSegDegenerate;
        else s.n = nt >= 1073741824.0 ? 1073741824 : (int)ceil(nt);
    }
    if (gate) *gate = g;
    return s;
}
// (int) of a double as an x86-64 build converts it (cvttsd2si): INT_MIN outside the range
REBVO_SEG_HD int seg_d2i(double q) { return (q > -2147483649.0 && q < 2147483648.0) ? (int)q : (int)0x80000000; }
// depth_filler::getImgPoint((int)q[0], (int)q[1]) (depth_filler.h:197-201): the division is unsigned (bl_size is u_int), the clamp int
REBVO_SEG_HD int seg_cell_axis(int x, int bl, int g) {
    const int h = (int)((uint32_t)x / (uint32_t)bl);
    return h > g - 1 ? g - 1 : (h < 0 ? 0 : h);
}
REBVO_SEG_HD int seg_step_cell(const SegSteps &s, int i, int bw, int bh, int gw, int gh) {
    const double qx = s.q0x + s.tx * i, qy = s.q0y + s.ty * i;
    return seg_cell_axis(seg_d2i(qy), bh, gh) * gw + seg_cell_axis(seg_d2i(qx), bw, gw);
}
REBVO_SEG_HD double seg_step_rho(const SegSteps &s, int i) { return s.r1 * i + s.rho0; }

// the information-form update of one cell by one step (the fold FillEdgeData has too)
REBVO_SEG_HD void seg_fold(double rho, double kl_I, double *c_rho, double *c_srho, double *c_I) {
    double i_rho = *c_I * *c_rho;
    i_rho += rho * kl_I;
    *c_I += kl_I;
    const double v = *c_I > 0 ? 1.0 / *c_I : 1e20;
    *c_rho = i_rho * v;
    *c_srho = sqrt(v);
}

}  // namespace edgemap
}  // namespace rebvo
