// Driver of the reference's re-localisation for tools/make_keyframe_reloc_golden.py (build machine only, never shipped).
//
// Compiled into a temporary directory outside the repository, together with the reference's src/mtracklib/keyframe.cpp and
// src/visualizer/depth_filler.cpp, in place; the reference's src/mtracklib/kfvo.cpp is #included below (the function under test), and
// src/mtracklib/global_tracker.cpp comes with it the same way; everything else comes from oracle/_ref/libreforacle.so, as in
// tools/keyframe_covis_ref_driver.cpp.
//
// It builds M keyframe objects from records, each one's field with global_tracker::build_field(edges, radius, min_mod), and for every
// listed (query, key frame) pair runs kfvo::OptimizePosGT(kf_t, et, Pose, Pos, K, iter_max, rew_dis, rho_tol, s_rho_q, mnum, X, RRV) on a
// copy of the query's list with the query's pose.
//
// stdin : int32 M, w, h, radius, iter_max, npairs; float min_mod, ppx, ppy, zfx, zfy; double rew_dis, rho_tol, s_rho_q;
//         per key frame: int32 kn, pad; double Pose[9], Pos[3], K; kn x 168-byte KeyLine records;  int32 pairs[npairs][2] (query, key frame)
// stdout: per pair: int32 mnum, kn; double r, K, X[6], RRV[36], Pose[9], Pos[3]; int32 m_id_f[kn]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mtracklib/edge_tracker.h"
#include "mtracklib/global_tracker.h"
#include "src/mtracklib/kfvo.cpp"
#include "src/mtracklib/global_tracker.cpp"

using namespace rebvo;
using namespace TooN;

static bool rd(void *p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }

int main() {
    int32_t hdr[6];
    float fl[5];
    double dd[3];
    if (!rd(hdr, sizeof hdr) || !rd(fl, sizeof fl) || !rd(dd, sizeof dd)) return 2;
    const int M = hdr[0], w = hdr[1], h = hdr[2], radius = hdr[3], iter_max = hdr[4], npairs = hdr[5];
    static_assert(sizeof(KeyLine) == 168, "KeyLine layout");
    cam_model::rad_tan_distortion kc = {0, 0, 0, 0, 0};
    Size2D sz = {(unsigned)w, (unsigned)h};
    cam_model cam({fl[1], fl[2]}, {fl[3], fl[4]}, kc, sz);
    std::vector<keyframe> kfs;
    kfs.reserve(M);
    for (int m = 0; m < M; m++) {
        int32_t kh[2];
        double d[13];
        if (!rd(kh, sizeof kh) || !rd(d, sizeof d)) return 3;
        edge_tracker et(cam, 255 * 3, kh[0] > 0 ? kh[0] : 1);
        if (!rd(et.kl, sizeof(KeyLine) * (size_t)kh[0])) return 4;
        et.kn = kh[0];
        et.kl_size = kh[0];   // (the copy constructor sizes the copy by KNum())
        Matrix<3, 3> Pose;
        Vector<3> Pos;
        for (int i = 0; i < 9; i++) Pose(i / 3, i % 3) = d[i];
        for (int i = 0; i < 3; i++) Pos[i] = d[9 + i];
        global_tracker gt(cam);
        kfs.emplace_back(et, gt, 0.0, d[12], Identity, Zeros, Zeros, Pose, Zeros, Pos);
    }
    for (keyframe &kf : kfs) kf.tracker().build_field(kf.edges(), radius, fl[0]);
    std::vector<int32_t> pairs((size_t)npairs * 2);
    if (!rd(pairs.data(), pairs.size() * 4)) return 5;
    for (int p = 0; p < npairs; p++) {
        keyframe &q = kfs[pairs[2 * p]], &t = kfs[pairs[2 * p + 1]];
        edge_tracker et(q.edges());
        Matrix<3, 3> Pose = q.Pose;
        Vector<3> Pos = q.Pos;
        double K = q.K;
        int mnum = 0;
        Vector<6> X = Zeros;
        Matrix<6> RRV = Zeros;
        const double r = kfvo::OptimizePosGT(t, et, Pose, Pos, K, iter_max, dd[0], dd[1], dd[2], mnum, X, RRV);
        int32_t head[2] = {mnum, et.KNum()};
        fwrite(head, 4, 2, stdout);
        std::vector<double> o;
        o.push_back(r); o.push_back(K);
        for (int i = 0; i < 6; i++) o.push_back(X[i]);
        for (int i = 0; i < 36; i++) o.push_back(RRV(i / 6, i % 6));
        for (int i = 0; i < 9; i++) o.push_back(Pose(i / 3, i % 3));
        for (int i = 0; i < 3; i++) o.push_back(Pos[i]);
        fwrite(o.data(), 8, o.size(), stdout);
        for (int i = 0; i < et.KNum(); i++) { int32_t m = et[i].m_id_f; fwrite(&m, 4, 1, stdout); }
    }
    return 0;
}
