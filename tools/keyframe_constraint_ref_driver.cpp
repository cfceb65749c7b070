// Driver of the reference's key-frame relative-pose constraint for tools/make_keyframe_constraint_golden.py and
// tools/keyframe_constraint_timing.py (build machine only, never shipped).
//
// Compiled into a temporary directory outside the repository, together with the reference's src/mtracklib/keyframe.cpp and
// src/visualizer/depth_filler.cpp, in place; the reference's src/mtracklib/kfvo.cpp is #included below (the functions under test);
// everything else comes from oracle/_ref/libreforacle.so.  The generator pre-includes a header that declares std::max(float, double), as
// tools/make_keyframe_track_golden.py does.
//
// It builds the key frame and the frame (as a second keyframe object: mutualExclusionSimple takes two) from records, optionally runs
//   kfvo::mutualExclusionSimple(kf, frame, dist_t, discard, true)  and / or  (kf, frame, dist_t, discard, false)      (in that order)
// and then kfvo::OptimizeRelContraint(kf, frame.edges(), Pose, Pos, K, iter_max, X, W_X, R_X, optimK, direction, k_huber, match_num).
// E0 is not among that function's outputs: the driver repeats its first two evaluations (OptimizeRelConstraint1Iter at the start pose,
// kfvo.cpp:538-554) on its own.
//
// stdin : int32 kf_kn, fr_kn, direction, iter_max (< 0: pruning alone), prune (bit 0: kf -> frame, bit 1: frame -> kf), discard;
//         float ppx, ppy, zfx, zfy; int32 w, h; double k_huber, dist_t, kf_Pose[9], kf_Pos[3], kf_K, Pose[9], Pos[3], K;
//         kf_kn x 168-byte KeyLine records, fr_kn x 168-byte records
// stdout: int32 links, inliers, prune counts[4] (seen, kept of either pass), sizeof(sqrt(float)) as util::norm binds it, pad;
//         double X[6], W_X[36], R_X[36], ratio, E0, Kp, W_Kp, seconds; int32 m_id_f[kf_kn], m_id_kf[fr_kn] as the calls left them
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mtracklib/edge_tracker.h"
#include "mtracklib/global_tracker.h"
#include "src/mtracklib/kfvo.cpp"

namespace rebvo {
namespace util {
// the width of what util::norm<float>'s sqrt(norm2(a, b)) returns, in that header's own scope (UtilLib/util.h:118-121)
static int sqrt_width() { float a = 2.f; return (int)sizeof(sqrt(a)); }
}
}

using namespace rebvo;
using namespace TooN;

static bool rd(void *p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main() {
    int32_t hdr[6], wh[2];
    float fl[4];
    double d[2 + 13 + 13];
    if (!rd(hdr, sizeof hdr) || !rd(fl, sizeof fl) || !rd(wh, sizeof wh) || !rd(d, sizeof d)) return 2;
    const int kf_kn = hdr[0], fr_kn = hdr[1], iter_max = hdr[3], prune = hdr[4];
    const bool direction = hdr[2] != 0, discard = hdr[5] != 0;
    static_assert(sizeof(KeyLine) == 168, "KeyLine layout");
    cam_model::rad_tan_distortion kc = {0, 0, 0, 0, 0};
    Size2D sz = {(unsigned)wh[0], (unsigned)wh[1]};
    cam_model cam({fl[0], fl[1]}, {fl[2], fl[3]}, kc, sz);
    std::vector<keyframe> kfs;
    kfs.reserve(2);
    Matrix<3, 3> P[2];
    Vector<3> T[2];
    double K[2];
    for (int m = 0; m < 2; m++) {
        const double *q = d + 2 + 13 * m;
        for (int i = 0; i < 9; i++) P[m](i / 3, i % 3) = q[i];
        for (int i = 0; i < 3; i++) T[m][i] = q[9 + i];
        K[m] = q[12];
    }
    for (int m = 0; m < 2; m++) {
        const int kn = m ? fr_kn : kf_kn;
        edge_tracker et(cam, 255 * 3, kn > 0 ? kn : 1);
        if (!rd(et.kl, sizeof(KeyLine) * (size_t)kn)) return 4;
        et.kn = kn;
        et.kl_size = kn;   // (the copy constructor sizes the copy by KNum())
        global_tracker gt(cam);
        kfs.emplace_back(et, gt, 0.0, K[m], Identity, Zeros, Zeros, P[m], Zeros, T[m]);
    }
    keyframe &kf = kfs[0], &fr = kfs[1];
    int32_t head[8] = {0, 0, 0, 0, 0, 0, util::sqrt_width(), 0};
    if (prune & 1) { std::pair<int, int> c = kfvo::mutualExclusionSimple(kf, fr, d[1], discard, true); head[2] = c.first; head[3] = c.second; }
    if (prune & 2) { std::pair<int, int> c = kfvo::mutualExclusionSimple(kf, fr, d[1], discard, false); head[4] = c.first; head[5] = c.second; }
    double res[6 + 36 + 36 + 5];
    memset(res, 0, sizeof res);
    if (iter_max >= 0) {
        Vector<6> X;
        Matrix<6, 6> W_X, R_X;
        std::pair<double, double> optimK(0, 0);
        std::pair<int, int> match_num(0, 0);
        const double t0 = now();
        const double ratio = kfvo::OptimizeRelContraint(kf, fr.edges(), P[1], T[1], K[1], iter_max, X, W_X, R_X, optimK, direction, d[0], match_num);
        res[82] = now() - t0;
        for (int i = 0; i < 6; i++) res[i] = X[i];
        for (int i = 0; i < 36; i++) { res[6 + i] = W_X(i / 6, i % 6); res[42 + i] = R_X(i / 6, i % 6); }
        res[78] = ratio; res[80] = optimK.first; res[81] = optimK.second;
        head[0] = match_num.first; head[1] = match_num.second;
        {   // E0: the function's first two evaluations again (kfvo.cpp:538-554)
            Matrix<3, 3> BRelRot;
            Vector<3> BRelPos;
            if (direction) { BRelRot = kf.Pose.T() * P[1]; BRelPos = kf.Pose.T() * (T[1] - kf.Pos) / K[1]; }
            else { BRelRot = P[1].T() * kf.Pose; BRelPos = P[1].T() * (kf.Pos - T[1]) / kf.K; }
            const int kl_num = direction ? fr.edges().KNum() : kf.edges().KNum();
            Vector<Dynamic> residual(kl_num);
            residual = Zeros;
            Matrix<6, 6> JtJ;
            Vector<6> JtF;
            std::pair<int, int> mn;
            kfvo::OptimizeRelConstraint1Iter(kf, fr.edges(), BRelRot, BRelPos, JtJ, JtF, direction, d[0], residual, mn);
            res[79] = kfvo::OptimizeRelConstraint1Iter(kf, fr.edges(), BRelRot, BRelPos, JtJ, JtF, direction, d[0], residual, mn);
        }
    }
    fwrite(head, 4, 8, stdout);
    fwrite(res, 8, 83, stdout);
    std::vector<int32_t> f(kf_kn), b(fr_kn);
    for (int i = 0; i < kf_kn; i++) f[i] = kf.edges()[i].m_id_f;
    for (int i = 0; i < fr_kn; i++) b[i] = fr.edges()[i].m_id_kf;
    fwrite(f.data(), 4, f.size(), stdout);
    fwrite(b.data(), 4, b.size(), stdout);
    return 0;
}
