// edgemap_fit.h — the reference's polyline edge map, edgemap_com_sender::compress_edgemap (src/CommLib/edgemap_com.cpp:162-326) with
// LineFitting::RobustFit3DLine<float> and Fit2DLine<float, double> under it (src/UtilLib/linefitting.cpp:12-43, 111-204): the walk of ONE
// head and the fit, written once for the device kernels (edgemap_compress.hip), the serial host restatement (rebvo/edgemap_com.h) and
// the tools.  Header-only, __host__ __device__, no library call but sqrt: host and device run the same IEEE operations in the same order
// (every user compiles with -ffp-contract=off).
//
// The KeyLines are read through an accessor KL:
//     int kn();  int next(int k);  int prev(int k);      links already confined to [-1, kn): anything else reads as -1 (link_in_range)
//     float cx(k), cy(k), ux(k), uy(k);                  c_p, u_m
//     double rho(k), s_rho(k);  int m_num(k);
// the reference's kl_mask through Mask { bool get(k); void set(k); void clear(k); }, and records leave through Out { put(int i, Rec) }
// with i counted from the walk's first record; Out::kFit == false makes a walk that only counts (no fit is computed: no decision of the
// walk depends on a fit's result).
//
// The fit list is never stored.  The reference appends k_next to fit_list at every step and restarts the list at a cut with the cut
// KeyLine, so at any moment the list is the n_id path of f_inx KeyLines that starts at k_break; the fit and the final unmasking walk that
// path again.  Nothing limits max_line_len.
//
// The angle.  Fit2DLine takes a = 0.5 * atan2(-2 Sxy, Sxx - Syy) and uses sin a, cos a.  half_angle() gets both from (X, Y) = (Sxx - Syy,
// -2 Sxy) by square roots and divisions: with r = |(X, Y)|, cos 2a = X / r, so for X >= 0 cos a = sqrt((r + X) / 2r), sin a = Y / (2 r cos a)
// and for X < 0 |sin a| = sqrt((r - X) / 2r) with Y's sign, cos a = |Y| / (2 r |sin a|).  Y == 0 keeps its sign: atan2(-0, X < 0) = -pi, so
// an exact vertical run has sin a = -1; cos a is there what glibc returns for cos(-pi/2 as a double), 6.123233995736766e-17 (pi/2 is not
// a double), and the reference's tx is that value narrowed to float, not 0.  X == Y == 0 (identical points) gives a = Y (a signed zero).
// Away from those cases the two forms can differ in the last bits of the double, before tx, ty and zfo are narrowed to float; the
// fixtures (tools/make_edgemap_golden.py) are refused when a narrowed value differs.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define REBVO_EM_HD __host__ __device__ inline
#else
#define REBVO_EM_HD inline
#endif

namespace rebvo {
namespace edgemap {

enum Status {
    kBadLink = 1,    // some p_id / n_id outside [-1, kn): read as -1
    kOverflow = 2,   // more records than the caller's span holds: count 0 (the reference's `return kl_num=0`)
    kStepGuard = 4   // a walk reached kn + 1 steps (cannot happen: every step masks a KeyLine that was unmasked, or ends the walk)
};

struct Rec {         // compressed_kl before it is packed into 5 bytes
    uint8_t x, y;
    int16_t rho;
    uint8_t s_rho;
};

struct WalkParams {
    int min_line_len, max_line_len, match_n_t;
    double max_cangle;           // cos(max_angle), computed once by the caller (edgemap_com.cpp:170)
    double rho_rel_max;
    double x_scaling, y_scaling; // COMPRESSED_X_SCALING 0.5, COMPRESSED_Y_SCALING 1 (edgemap_com.h:42-43)
    double scale;
    float ppx, ppy;              // cam_model::pp
    double zfm;                  // cam_model::zfm
};

struct FitTrace {    // what the fixture generator compares with the reference's Fit2DLine (may be null everywhere)
    int start, n;    // the fit list: the n_id path of n KeyLines from start
    float tx, ty, zfo;
    int flags;       // 1: the degenerate branch, 2: a residual above its s_rho, 4: neighbouring rho further apart than the smaller s_rho
};

REBVO_EM_HD int link_in_range(int v, int kn) { return (v >= 0 && v < kn) ? v : -1; }
REBVO_EM_HD bool link_is_bad(int v, int kn) { return v < -1 || v >= kn; }

// util::clamp_uchar / clamp_short (include/UtilLib/util.h:52-55, 68-76): the argument arrives as float, the conversion truncates
REBVO_EM_HD uint8_t clamp_uchar(float f) { return f < 0 ? (uint8_t)0 : f > 255.0f ? (uint8_t)255 : (uint8_t)(int)f; }
REBVO_EM_HD int16_t clamp_short(float f) { return f < -32768.0f ? (int16_t)-32768 : f > 32767.0f ? (int16_t)32767 : (int16_t)(int)f; }

REBVO_EM_HD float rho_scaling() { return (float)(32767.0 / 20); }    // COMPRESSED_RHO_SCALING
REBVO_EM_HD float srho_scaling() { return (float)(255.0 / 20); }     // COMPRESSED_SRHO_SCALING

// edgemap_com.cpp:240-243: x * 0.5 in double, y * 1 (exact in either type), rho * scaling in float, / scale in double, max with
// COMPRESSED_RHO_MIN in double, sigma * scaling in double; every product is narrowed to float on its way into the clamp
REBVO_EM_HD Rec make_rec(const float p[3], double sigma, const WalkParams &P) {
    Rec r;
    r.x = clamp_uchar((float)((double)p[0] * P.x_scaling));
    r.y = clamp_uchar((float)((double)p[1] * P.y_scaling));
    const double v = (double)(p[2] * rho_scaling()) / P.scale, floor_ = (double)rho_scaling() * 1e-3;
    r.rho = clamp_short((float)(v < floor_ ? floor_ : v));
    r.s_rho = clamp_uchar((float)(sigma * (double)srho_scaling()));
    return r;
}

// sin a, cos a of a = 0.5 * atan2(Y, X) (see the head of the file)
REBVO_EM_HD void half_angle(double X, double Y, double &s, double &c) {
    const double r = sqrt(X * X + Y * Y);
    if (r == 0) { s = Y; c = 1; return; }
    if (X >= 0) {
        c = sqrt((r + X) / (2 * r));
        s = Y / (2 * r * c);
    } else {
        const double as = sqrt((r - X) / (2 * r));
        s = signbit(Y) ? -as : as;
        c = Y == 0 ? 6.123233995736766e-17 : fabs(Y) / (2 * r * as);
    }
}

template <class KL> REBVO_EM_HD float fit_s_rho(const KL &kl, int k, int match_n_t) {
    return kl.m_num(k) >= match_n_t ? (float)kl.s_rho(k) : 1e10f;
}

// RobustFit3DLine<float> on the n_id path of n KeyLines from `start`.  p0 / p1 = {x, y, rho}; returns fit_sigma.
template <class KL>
REBVO_EM_HD double robust_fit(const KL &kl, const WalkParams &P, int start, int n, float p0[3], float p1[3], FitTrace *trace) {
    // Fit2DLine: means, then second moments of the float-narrowed offsets, all sums in double in list order
    double m_x = 0, m_y = 0;
    float mean_s = 0;
    float hx0 = 0, hy0 = 0, hxl = 0, hyl = 0, rho0 = 0, rhol = 0;
    int k = start;
    for (int i = 0; i < n; i++) {
        const float hx = kl.cx(k) - P.ppx, hy = kl.cy(k) - P.ppy;   // cam.Img2Hom, in place in the reference
        m_x += hx; m_y += hy;
        mean_s += fit_s_rho(kl, k, P.match_n_t);
        if (i == 0) { hx0 = hx; hy0 = hy; rho0 = (float)kl.rho(k); }
        if (i == n - 1) { hxl = hx; hyl = hy; rhol = (float)kl.rho(k); }
        else k = kl.next(k);
    }
    m_x /= n; m_y /= n;
    mean_s /= n;
    double Sxx = 0, Syy = 0, Sxy = 0;
    k = start;
    for (int i = 0; i < n; i++) {
        const float hx = kl.cx(k) - P.ppx, hy = kl.cy(k) - P.ppy;
        const float x = (float)(hx - m_x), y = (float)(hy - m_y);
        Sxx += x * x; Sxy += x * y; Syy += y * y;                   // float products
        if (i < n - 1) k = kl.next(k);
    }
    double m1, m2;
    half_angle(Sxx - Syy, -2 * Sxy, m1, m2);
    const double m3 = -(m1 * m_x + m2 * m_y);
    const float tx = (float)m2, ty = (float)(-m1);
    const float zfo = (float)sqrt(P.zfm * P.zfm + m3 * m3);
    if (trace) { trace->start = start; trace->n = n; trace->tx = tx; trace->ty = ty; trace->zfo = zfo; trace->flags = 0; }
    // the 2 x 2 normal equations (w = 1), TooN's dot products: from 0, ascending
    double Pi00 = 0, Pi01 = 0, Pi10 = 0, Pi11 = 0, b0 = 0, b1 = 0;
    float ql0 = 0, qll = 0;
    k = start;
    for (int i = 0; i < n; i++) {
        const float hx = kl.cx(k) - P.ppx, hy = kl.cy(k) - P.ppy;
        const float ql = hx * tx + hy * ty, s = fit_s_rho(kl, k, P.match_n_t);
        const double a = ql / P.zfm / s, b = zfo / P.zfm / s, y = (float)kl.rho(k) / s;   // Y[i]: a float quotient
        Pi00 += a * a; Pi01 += a * b; Pi10 += b * a; Pi11 += b * b;
        b0 += a * y; b1 += b * y;
        if (i == 0) ql0 = ql;
        if (i == n - 1) qll = ql;
        else k = kl.next(k);
    }
    if (Pi00 * Pi11 - Pi10 * Pi01 < 1e-10) {   // p0 = plist[0], p1 = plist[size-1]: still in homogeneous coordinates
        p0[0] = hx0; p0[1] = hy0; p0[2] = rho0;
        p1[0] = hxl; p1[1] = hyl; p1[2] = rhol;
        if (trace) trace->flags = 1;
        return 1e10;
    }
    const double d = 1. / (Pi00 * Pi11 - Pi10 * Pi01);   // TooN::inv(Matrix<2>)
    const double P00 = Pi11 * d, P01 = -Pi01 * d, P10 = -Pi10 * d, P11 = Pi00 * d;
    const double R0 = 0.0 + P00 * b0 + P01 * b1, R1 = 0.0 + P10 * b0 + P11 * b1;
    const double Q1 = zfo / P.zfm;
    p0[2] = (float)(0.0 + ql0 / P.zfm * R0 + Q1 * R1);
    p1[2] = (float)(0.0 + qll / P.zfm * R0 + Q1 * R1);
    p0[0] = hx0 + P.ppx; p0[1] = hy0 + P.ppy;           // cam.Hom2Img
    p1[0] = hxl + P.ppx; p1[1] = hyl + P.ppy;
    int bad = 0;
    float rho_prev = 0, s_prev = 0;
    k = start;
    for (int i = 0; i < n; i++) {
        const float hx = kl.cx(k) - P.ppx, hy = kl.cy(k) - P.ppy;
        const float ql = hx * tx + hy * ty, s = fit_s_rho(kl, k, P.match_n_t), rho = (float)kl.rho(k);
        const double r = fabs(rho - (ql / P.zfm * R0 + zfo / P.zfm * R1));
        if (r > s) bad |= 2;
        if (i > 0 && fabsf(rho_prev - rho) > (s < s_prev ? s : s_prev)) bad |= 4;   // std::min(plist[i].s_rho, plist[i+1].s_rho)
        rho_prev = rho; s_prev = s;
        if (i < n - 1) k = kl.next(k);
    }
    if (trace) trace->flags = bad;
    return bad ? 1e10 : (double)mean_s;
}

// One head's walk (edgemap_com.cpp:188-314).  Returns the number of records it wrote (out.put(0 .. count-1)).
template <class KL, class Mask, class Out>
REBVO_EM_HD int walk_head(const KL &kl, Mask &mask, const WalkParams &P, int head, Out &out, int &status, FitTrace *trace = nullptr, int *ntrace = nullptr) {
    const int kn = kl.kn();
    int c = 0, line_len = 0, k_break = head, k_next = head, f_inx = 1, steps = 0;
    bool breaked = false;
    Rec pend = {0, 0, 0, 0};
    float p0[3], p1[3];
    while (f_inx < P.max_line_len) {
        const int nx = kl.next(k_next);
        if (nx == -1) break;
        if (++steps > kn + 1) { status |= kStepGuard; break; }
        line_len++;
        const int k_prev = k_next;
        k_next = nx;
        if (mask.get(k_next)) break;
        const double rp = kl.rho(k_prev), rn = kl.rho(k_next);
        if (rp / rn > P.rho_rel_max || rn / rp > P.rho_rel_max) break;
        f_inx++;
        if (line_len > P.min_line_len && (double)(kl.ux(k_break) * kl.ux(k_next) + kl.uy(k_break) * kl.uy(k_next)) < P.max_cangle) {
            if (Out::kFit) {
                const double sigma = robust_fit(kl, P, k_break, f_inx, p0, p1, trace ? trace + (*ntrace)++ : nullptr);
                out.put(c, make_rec(p0, sigma, P));
                pend = make_rec(p1, sigma, P);   // kls[c_inx] after the increment: the next vertex written there replaces it
            }
            c++;
            f_inx = 1;
            k_break = k_next;
            line_len = 0;
            breaked = true;
        }
        mask.set(k_next);
    }
    if (line_len > P.min_line_len) {
        if (Out::kFit) {
            const double sigma = robust_fit(kl, P, k_break, f_inx, p0, p1, trace ? trace + (*ntrace)++ : nullptr);
            out.put(c, make_rec(p0, sigma, P));
            Rec e = make_rec(p1, sigma, P);
            e.rho = (int16_t)-e.rho;
            out.put(c + 1, e);
        }
        c += 2;
        f_inx = 0;
    } else if (breaked) {
        if (Out::kFit) {
            pend.rho = (int16_t)-pend.rho;
            out.put(c, pend);
        }
        c++;
    }
    for (int i = 0, k = k_break; i < f_inx; i++) {   // the KeyLines still in the fit list lose their mask bit
        mask.clear(k);
        if (i < f_inx - 1) k = kl.next(k);
    }
    return c;
}

struct CountOnly {
    enum { kFit = 0 };
    REBVO_EM_HD void put(int, const Rec &) {}
};

}  // namespace edgemap
}  // namespace rebvo
