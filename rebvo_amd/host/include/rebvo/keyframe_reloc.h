// keyframe_reloc.h — kfvo::OptimizePosGT (src/mtracklib/kfvo.cpp:58-112) as one plain serial C++ statement for ONE (query, key frame) pair, on
// top of linalg.h: global_tracker::build_field (global_tracker.cpp:61-105), kfvo::Minimizer_RV_KF<double,false> (:1679-1825) with
// kfvo::TryVelRot<double,true,true,false> (:1389-1668) and Calc_f_J_Complete<double> (global_tracker.cpp:116-165), kfvo::optimizeScale
// (:222-260) and the returned pose (:89-96).  What libedgehip's edgehip_keyframe_relocalize computes for a batch on the device
// (include/edgehip.h), in the reference's order of operations: the 28 sums of an evaluation are Ne10::DotProduct's — the
// products, padded with zeros to a multiple of four, added by PairWiseVAdd's halving (ne10wrapper.h:333-361); optimizeScale's two sums
// are running sums in KeyLine order.  Used by tests/test_keyframe_reloc_cpu.py through rebvo_keyframe_relocalize_c (librebvohost.so) and
// by tools/keyframe_reloc_guard.cpp.
//
// An empty query returns score_ratio = 0, mnum = 0, Kp = 1, X = [BRelPos, W0], RRV = 0 and the pose from the unchanged W0 / BRelPos.
// Non-finite inputs form no index: a KeyLine whose projection is not a number counts as outside the image.
#ifndef REBVO_KEYFRAME_RELOC_H
#define REBVO_KEYFRAME_RELOC_H

#include <cmath>
#include <cstdint>
#include <vector>

#include "rebvo/linalg.h"

namespace rebvo {

struct RelocKeyLines {   // a KeyLine list as the eleven numbers the rule reads, [kn] each (p_m, c_p, u_m, m_m as x, y pairs)
    int kn;
    const float *p_m, *c_p, *u_m, *m_m, *n_m;
    const double *rho, *s_rho;
};
struct RelocCamera { int w, h; float ppx, ppy; double zfm; };
struct RelocArgs { int field_radius; float field_min_mod; int iter_max; double rew_dis, rho_tol, s_rho_q; };
struct RelocResult {
    double X[6], RRV[36], score_ratio, F, F0, Kp, K, Pose[9], Pos[3];
    int mnum, evals, accepted;
};

namespace reloc_detail {

inline double pairwise_add(std::vector<double> v) {   // Ne10::PairWiseVAdd over a list already padded to a multiple of four
    int n = (int)v.size();
    double odd = 0;
    while (n > 3) {
        odd += (n & 1) ? v[(size_t)n - 1] : 0;
        n >>= 1;
        for (int i = 0; i < n; i++) v[(size_t)i] = v[(size_t)i] + v[(size_t)(i + n)];
    }
    for (int i = 0; i < n; i++) odd += v[(size_t)i];
    return odd;
}

// build_field: ikl ascending, t over [-radius, radius); a cell is overwritten when |t| <= its dist
inline std::vector<int> build_field(const RelocKeyLines &k, const RelocCamera &c, int radius, float min_mod) {
    std::vector<int> ikl((size_t)c.w * c.h, -1), dist((size_t)c.w * c.h, 0);
    for (int i = 0; i < k.kn; i++) {
        if (min_mod > 0 && k.n_m[i] < min_mod) continue;
        for (int t = -radius; t < radius; t++) {
            const float fx = k.u_m[2 * i] * (float)t + k.c_p[2 * i], fy = k.u_m[2 * i + 1] * (float)t + k.c_p[2 * i + 1];
            const float rx = std::round(fx), ry = std::round(fy);
            if (!(rx >= 0.f && rx < (float)c.w && ry >= 0.f && ry < (float)c.h)) continue;
            const size_t at = (size_t)(int)ry * c.w + (size_t)(int)rx;
            const int a = t < 0 ? -t : t;
            if (ikl[at] < 0 || a <= dist[at]) { ikl[at] = i; dist[at] = a; }
        }
    }
    return ikl;
}

struct Eval { double F; la::Mat<6, 6> JtJ; la::Vec<6> JtF; };

inline Eval try_vel_rot(const la::Vec<6> &X, const RelocKeyLines &q, const RelocKeyLines &kf, const std::vector<int> &field, const RelocCamera &cam,
                        double Kr, double match_mod, double match_cang, double rho_tol, double s_rho_min, double k_huber, double max_r,
                        const std::vector<double> &resid, std::vector<double> &resid_new, std::vector<int32_t> &m_id_f) {
    const int kn = q.kn, pnum = (kn + 3) & ~3;
    const la::Mat<3, 3> R = la::so3_exp(la::Vec<3>{{X[3], X[4], X[5]}});
    std::vector<double> J[6], fm((size_t)pnum, 0.0);
    for (auto &j : J) j.assign((size_t)pnum, 0.0);
    double fi = 0;
    for (int i = 0; i < kn; i++) {
        m_id_f[(size_t)i] = -1;
        const double s_rho = q.s_rho[i];
        if (s_rho > s_rho_min) continue;
        const double rho0 = q.rho[i], z = 1.0 / rho0, zz = z / cam.zfm;
        const double P0[3] = {zz * (double)q.p_m[2 * i], zz * (double)q.p_m[2 * i + 1], z};
        double Pt[3];
        for (int r = 0; r < 3; r++) Pt[r] = (R(r, 0) * P0[0] + R(r, 1) * P0[1]) + R(r, 2) * P0[2] + X[r];
        const double rho_p = 1.0 / Pt[2], pz = cam.zfm * rho_p, pix = pz * Pt[0], piy = pz * Pt[1];
        const double px = pix + (double)cam.ppx, py = piy + (double)cam.ppy;
        double weight = 1;
        if (std::fabs(resid[(size_t)i]) > k_huber) weight = k_huber / std::fabs(resid[(size_t)i]);
        double f = max_r, dfx = 0, dfy = 0;
        const double xr = px + 0.5, yr = py + 0.5;
        const bool in = xr >= 1.0 && yr >= 1.0 && xr < (double)(cam.w - 1) + 0.0 && yr < (double)(cam.h - 1) + 0.0 && (int)xr >= 1 && (int)yr >= 1 &&
                        (int)xr < cam.w - 1 && (int)yr < cam.h - 1;   // NaN fails every comparison: outside, and no index is formed
        if (!in) {
            resid_new[(size_t)i] = max_r;
        } else {
            const int b = field[(size_t)(int)yr * cam.w + (size_t)(int)xr];
            if (b >= 0) {
                const double cang = (double)((q.m_m[2 * i] * kf.m_m[2 * b] + q.m_m[2 * i + 1] * kf.m_m[2 * b + 1]) / q.n_m[i]);
                const double rho_t = rho_p / Kr;
                const bool rej = cang < match_cang || (double)std::fabs(q.n_m[i] / kf.n_m[b] - 1.f) > match_mod ||
                                 std::fabs(rho_t - kf.rho[b]) > rho_tol * (kf.s_rho[b] + s_rho * rho_t / rho0);
                if (!rej) {
                    fi = (px - (double)kf.c_p[2 * b]) * (double)kf.u_m[2 * b] + (py - (double)kf.c_p[2 * b + 1]) * (double)kf.u_m[2 * b + 1];
                    f = fi; dfx = (double)kf.u_m[2 * b]; dfy = (double)kf.u_m[2 * b + 1];
                    m_id_f[(size_t)i] = b;
                }
            }
            resid_new[(size_t)i] = fi;
        }
        f *= weight; dfx *= weight; dfy *= weight;
        double Jr[6];
        const double t0 = cam.zfm * rho_p;
        Jr[0] = t0 * dfx; Jr[1] = t0 * dfy;
        Jr[2] = (rho_p * pix) * dfx + (rho_p * piy) * dfy;
        Jr[3] = Jr[1] * Pt[2] + Jr[2] * Pt[1];
        Jr[4] = Jr[0] * Pt[2] + Jr[2] * Pt[0];
        Jr[5] = -1.0 * (Jr[0] * Pt[1]) + Jr[1] * Pt[0];
        const double qvel = cam.zfm * dfx * X[0] + cam.zfm * dfy * X[1] + (pix * dfx + piy * dfy) * X[2];
        const double q_rho = std::sqrt(s_rho * qvel * s_rho * qvel + 1);
        for (int j = 0; j < 6; j++) J[j][(size_t)i] = Jr[j] / q_rho;
        fm[(size_t)i] = f / q_rho;
    }
    Eval e;
    auto dotp = [&](const std::vector<double> &a, const std::vector<double> &b) {
        std::vector<double> p((size_t)pnum);
        for (int i = 0; i < pnum; i++) p[(size_t)i] = a[(size_t)i] * b[(size_t)i];
        return pairwise_add(p);
    };
    for (int i = 0; i < 6; i++) {
        for (int j = i; j < 6; j++) e.JtJ(i, j) = dotp(J[i], J[j]);
        e.JtF[i] = dotp(J[i], fm);
    }
    for (int i = 0; i < 2; i++) {
        e.JtF[i + 2] = -e.JtF[i + 2];
        for (int j = 0; j < 2; j++) { e.JtJ(i, j + 2) = -e.JtJ(i, j + 2); e.JtJ(i + 2, j + 4) = -e.JtJ(i + 2, j + 4); }
    }
    for (int i = 0; i < 6; i++)
        for (int j = i + 1; j < 6; j++) e.JtJ(j, i) = e.JtJ(i, j);
    e.F = dotp(fm, fm);
    return e;
}

}  // namespace reloc_detail

// query: KeyLines and (Pose, Pos, K); kf: key frame t's.  m_id_f: room for query.kn links (may be null).
inline void rebvo_keyframe_relocalize(const RelocKeyLines &query, const double Pose[9], const double Pos[3], double K, const RelocKeyLines &kf,
                                      const double Pose_t[9], const double Pos_t[3], double K_t, const RelocCamera &cam, const RelocArgs &a,
                                      RelocResult &out, int32_t *m_id_f) {
    using namespace reloc_detail;
    la::Mat<3, 3> Pq, Pt;
    la::Vec<3> d;
    for (int i = 0; i < 9; i++) { Pq.a[i] = Pose[i]; Pt.a[i] = Pose_t[i]; }
    for (int i = 0; i < 3; i++) d[i] = Pos[i] - Pos_t[i];
    const la::Mat<3, 3> PtT = la::transpose(Pt);
    const la::Vec<3> BRelPos = (PtT * d) / K;
    const la::Vec<3> W0 = la::so3_ln(PtT * Pq);
    la::Vec<6> X;
    for (int i = 0; i < 3; i++) { X[i] = BRelPos[i]; X[3 + i] = W0[i]; }
    const int kn = query.kn;
    std::vector<int32_t> mid((size_t)kn, -1);
    la::Mat<6, 6> RRV = la::Mat<6, 6>::zeros();
    double F = 0, F0 = 0, ratio = 0;
    int evals = 0, accepted = 0;
    if (kn > 0) {
        const std::vector<int> field = build_field(kf, cam, a.field_radius, a.field_min_mod);
        const double Kr = K / K_t, cang = std::cos(30.0 * M_PI / 180.0), max_r = (double)a.field_radius;
        std::vector<double> res((size_t)kn, 0.0), res_new((size_t)kn, 0.0);
        auto ev = [&](const la::Vec<6> &Xe) { evals++; return try_vel_rot(Xe, query, kf, field, cam, Kr, 5.0, cang, a.rho_tol, a.s_rho_q, a.rew_dis, max_r, res, res_new, mid); };
        Eval cur = ev(X);
        F0 = F = cur.F;
        double mx = cur.JtJ.a[0];
        for (int i = 1; i < 36; i++) mx = cur.JtJ.a[i] > mx ? cur.JtJ.a[i] : mx;
        double u = 1e-3 * mx, v = 2;
        for (int it = 0; it < a.iter_max; it++) {
            la::Mat<6, 6> ApI = cur.JtJ;
            la::Vec<6> nb;
            for (int i = 0; i < 6; i++) { ApI(i, i) = cur.JtJ(i, i) + 1.0 * u; nb[i] = -cur.JtF[i]; }
            const la::Vec<6> h = la::Cholesky<6>(ApI).backsub(nb);
            la::Vec<6> Xn;
            for (int i = 0; i < 6; i++) Xn[i] = X[i] + h[i];
            const Eval nw = ev(Xn);
            double den = 0;
            for (int i = 0; i < 6; i++) den += (0.5 * h[i]) * (u * h[i] - cur.JtF[i]);
            const double gain = (F - nw.F) / den;
            if (gain > 0) {
                F = nw.F; X = Xn; cur = nw;
                const double g = 2 * gain - 1, m = 1 - g * g * g;
                u *= (0.33 > m ? 0.33 : m);
                v = 2;
                accepted++;
                res.swap(res_new);
            } else {
                u *= v;
                v *= 2;
            }
        }
        RRV = la::Cholesky<6>(cur.JtJ).inverse();
        ratio = F / F0;
    }
    // optimizeScale
    const la::Mat<3, 3> R = la::so3_exp(la::Vec<3>{{X[3], X[4], X[5]}});
    double rTr = 0, rTr0 = 0;
    int mnum = 0;
    for (int i = 0; i < kn; i++) {
        const int b = mid[(size_t)i];
        if (m_id_f) m_id_f[i] = b;
        if (b < 0) continue;
        mnum++;
        const double ir = 1 / query.rho[i];
        const la::Vec<3> uu = {{((double)query.p_m[2 * i] / cam.zfm) * ir, ((double)query.p_m[2 * i + 1] / cam.zfm) * ir, 1.0 * ir}};
        const la::Vec<3> p = R * uu + la::Vec<3>{{X[0], X[1], X[2]}};
        const double q2 = 1.0 * (1 / p[2]);
        if (q2 > 0) {
            const double vv = query.s_rho[i] * query.s_rho[i] * 1.0 * 1.0 + kf.s_rho[b] * kf.s_rho[b];
            rTr0 += q2 * q2 / vv;
            rTr += q2 * kf.rho[b] / vv;
        }
    }
    out.Kp = (rTr0 > 0 && rTr > 0) ? rTr0 / rTr : 1;
    out.K = K_t * out.Kp;
    const la::Mat<3, 3> Pc = la::so3_coerce(Pt), Po = Pc * R;
    const la::Vec<3> pr = (Pc * la::Vec<3>{{X[0], X[1], X[2]}}) * out.K;
    for (int i = 0; i < 6; i++) out.X[i] = X[i];
    for (int i = 0; i < 36; i++) out.RRV[i] = RRV.a[i];
    for (int i = 0; i < 9; i++) out.Pose[i] = Po.a[i];
    for (int i = 0; i < 3; i++) out.Pos[i] = pr[i] + Pos_t[i];
    out.score_ratio = ratio; out.F = F; out.F0 = F0;
    out.mnum = mnum; out.evals = evals; out.accepted = accepted;
}

}  // namespace rebvo
#endif
