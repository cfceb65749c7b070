// Stand-alone guard of rebvo/keyframe_reloc.h (the host restatement of kfvo::OptimizePosGT): crafted and degenerate inputs under the host
// compiler's sanitizers.  Not loaded into Python, not run on a GPU.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -Irebvo_amd/host/include \
//       tools/keyframe_reloc_guard.cpp -o /tmp/keyframe_reloc_guard && /tmp/keyframe_reloc_guard
// Inputs (seeded): key-frame lists of 0, 1, 5, 65, 257, 600 and 1030 KeyLines at 70x50, the query the key frame with 0.3 px of noise and a tenth
// pushed off the image; then the degenerate ones: an empty query, NaN and infinite and zero rho, a NaN pose, KeyLines far outside the image,
// s_rho above the gate everywhere, iter_max 0.  Prints one line per case; the exit status is the sanitizers'.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "rebvo/keyframe_reloc.h"

struct List {
    std::vector<float> p_m, c_p, u_m, m_m, n_m;
    std::vector<double> rho, s_rho;
    rebvo::RelocKeyLines view() const { return {(int)n_m.size(), p_m.data(), c_p.data(), u_m.data(), m_m.data(), n_m.data(), rho.data(), s_rho.data()}; }
};

static List make(std::mt19937 &g, int kn, const rebvo::RelocCamera &c) {
    std::uniform_real_distribution<double> U(0, 1);
    List l;
    for (int i = 0; i < kn; i++) {
        const float x = (float)(U(g) * c.w - 0.4), y = (float)(U(g) * c.h - 0.4), ang = (float)(U(g) * 6.2831853), n = (float)(3 + 9 * U(g));
        l.c_p.push_back(x); l.c_p.push_back(y);
        l.p_m.push_back(x - c.ppx); l.p_m.push_back(y - c.ppy);
        l.u_m.push_back(std::cos(ang)); l.u_m.push_back(std::sin(ang));
        l.m_m.push_back(std::cos(ang) * n); l.m_m.push_back(std::sin(ang) * n);
        l.n_m.push_back(n);
        l.rho.push_back(0.3 + 1.2 * U(g)); l.s_rho.push_back(0.02 + 0.38 * U(g));
    }
    return l;
}

static void run(const char *name, const List &q, const List &t, const double *qp, const double *tp, const rebvo::RelocCamera &c, rebvo::RelocArgs a) {
    rebvo::RelocResult r;
    std::vector<int32_t> mid(q.n_m.size() + 1, -2);
    rebvo::rebvo_keyframe_relocalize(q.view(), qp, qp + 9, qp[12], t.view(), tp, tp + 9, tp[12], c, a, r, mid.data());
    for (size_t i = 0; i < q.n_m.size(); i++)
        if (mid[i] < -1 || mid[i] >= (int)t.n_m.size()) { std::printf("%s: link %zu out of range\n", name, i); std::abort(); }
    std::printf("%-28s kn_q %4zu kn_t %4zu mnum %4d evals %d accepted %d ratio %.6g Kp %.6g\n", name, q.n_m.size(), t.n_m.size(), r.mnum, r.evals,
                r.accepted, r.score_ratio, r.Kp);
}

int main() {
    const rebvo::RelocCamera cam = {70, 50, 34.3f, 25.6f, 61.0};
    const rebvo::RelocArgs a = {5, 0.f, 6, 2.0, 1.5, 0.39};
    std::mt19937 g(7);
    std::normal_distribution<float> N(0.f, 0.3f);
    const double tp[13] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.1, -0.2, 0.05, 0.9};
    const double qp[13] = {0.9998, -0.02, 0.01, 0.02, 0.9998, -0.01, -0.01, 0.01, 0.9999, 0.12, -0.21, 0.08, 1.2};
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    for (int kn : {0, 1, 5, 65, 257, 600, 1030}) {
        const List t = make(g, kn, cam);
        List q = t;
        for (int i = 0; i < kn; i++) {
            q.p_m[2 * i] += N(g); q.p_m[2 * i + 1] += N(g);
            if (i % 10 == 3) q.p_m[2 * i] = -cam.ppx - 4.f;
            q.c_p[2 * i] = q.p_m[2 * i] + cam.ppx; q.c_p[2 * i + 1] = q.p_m[2 * i + 1] + cam.ppy;
        }
        run("moved", q, t, qp, tp, cam, a);
        rebvo::RelocArgs a0 = a;
        a0.iter_max = 0;
        run("moved, iter_max 0", q, t, qp, tp, cam, a0);
        run("empty query", List(), t, qp, tp, cam, a);
        if (kn < 65) continue;
        List d = q;
        d.rho[5] = nan; d.rho[6] = inf; d.rho[7] = 0; d.rho[8] = -inf; d.rho[9] = 1e-300; d.rho[10] = -1e300;
        run("NaN / inf / zero rho", d, t, qp, tp, cam, a);
        d = q;
        for (int i = 0; i < kn; i += 3) { d.p_m[2 * i] = 3e38f; d.p_m[2 * i + 1] = -3e38f; }
        run("far outside the image", d, t, qp, tp, cam, a);
        double bad[13];
        for (int i = 0; i < 13; i++) bad[i] = qp[i];
        bad[4] = nan;
        run("NaN pose", q, t, bad, tp, cam, a);
        rebvo::RelocArgs ag = a;
        ag.s_rho_q = 0;
        run("every KeyLine above the gate", q, t, qp, tp, cam, ag);
        List tn = t;
        tn.c_p[0] = (float)nan; tn.u_m[3] = (float)inf;
        run("NaN in the key frame", q, tn, qp, tp, cam, a);
    }
    std::printf("keyframe_reloc_guard: done\n");
    return 0;
}
