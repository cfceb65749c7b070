// Driver of the reference's key-frame depth functions for tools/make_keyframe_depth_golden.py (build machine only, never shipped).
//
// Compiled into a temporary directory outside the repository, together with the reference's src/mtracklib/keyframe.cpp and
// src/visualizer/depth_filler.cpp, in place; the reference's src/mtracklib/kfvo.cpp is #included below (the functions under test)
// through the copy the generator puts into that temporary directory: as written, the file's two helpers isnan(double&) / isinf(double&)
// (kfvo.cpp:10-17) call THEMSELVES under a current libstdc++ (where isnan is no macro), so mapKLUsingIDK never returns from the third
// condition of its clamp chain; in the copy the two calls inside the helpers are std::isnan / std::isinf, nothing else differs and the
// line numbers stay.  Everything else comes from oracle/_ref/libreforacle.so.  The generator pre-includes a header that declares
// std::max(float, double), as tools/make_keyframe_track_golden.py does.
//
// It builds `nkf` keyframe objects from records and runs ONE of
//   mode 0   kfvo::mapKFUsingIDK(kf[0], kf[1].edges(), kf[1].Pose, kf[1].Pos, args[0], args[1], args[2])
//   mode 1   kfvo::translateDepth_F2KF(kf[0], kf[1].edges(), kf[1].Pose, kf[1].Pos, kf[1].K, flag)
//   mode 2   kfvo::translateDepth_KF2F(kf[0], kf[1].edges(), kf[1].Pose, kf[1].Pos, kf[1].K)
//   mode 3   kfvo::translateDepth_New2Old(kf, flag)                                                   (flag = iters)
// timing that call alone.  The functions print to stdout, so the results go to the file named by argv[1].
//
// stdin : int32 mode, nkf, flag, pad; float ppx, ppy, zfx, zfy; int32 w, h; double args[3];
//         then per keyframe: int32 kn, pad; double Pose[9], Pos[3], K; kn x 168-byte KeyLine records
// file  : int32 count (the function's return value, 0 for modes 0 and 3), pad; double K of kf[0] afterwards, seconds;
//         then per keyframe its kn x 168-byte records as the call left them
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mtracklib/edge_tracker.h"
#include "mtracklib/global_tracker.h"
#include "kfvo_terminating.cpp"

using namespace rebvo;
using namespace TooN;

static bool rd(void *p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char **argv) {
    if (argc < 2) return 1;
    int32_t hdr[4], wh[2];
    float fl[4];
    double args[3];
    if (!rd(hdr, sizeof hdr) || !rd(fl, sizeof fl) || !rd(wh, sizeof wh) || !rd(args, sizeof args)) return 2;
    const int mode = hdr[0], nkf = hdr[1], flag = hdr[2];
    static_assert(sizeof(KeyLine) == 168, "KeyLine layout");
    cam_model::rad_tan_distortion kc = {0, 0, 0, 0, 0};
    Size2D sz = {(unsigned)wh[0], (unsigned)wh[1]};
    cam_model cam({fl[0], fl[1]}, {fl[2], fl[3]}, kc, sz);
    std::vector<keyframe> kfs;
    kfs.reserve(nkf);
    std::vector<int> kns;
    for (int m = 0; m < nkf; m++) {
        int32_t kh[2];
        double q[13];
        if (!rd(kh, sizeof kh) || !rd(q, sizeof q)) return 3;
        const int kn = kh[0];
        Matrix<3, 3> P;
        Vector<3> T;
        for (int i = 0; i < 9; i++) P(i / 3, i % 3) = q[i];
        for (int i = 0; i < 3; i++) T[i] = q[9 + i];
        edge_tracker et(cam, 255 * 3, kn > 0 ? kn : 1);
        if (!rd(et.kl, sizeof(KeyLine) * (size_t)kn)) return 4;
        et.kn = kn;
        et.kl_size = kn;   // (the copy constructor sizes the copy by KNum())
        global_tracker gt(cam);
        kfs.emplace_back(et, gt, 0.0, q[12], Identity, Zeros, Zeros, P, Zeros, T);
        kns.push_back(kn);
    }
    if ((mode < 3 && nkf != 2) || mode < 0 || mode > 3) return 5;
    int32_t head[2] = {0, 0};
    double res[2] = {0, 0};
    const double t0 = now();
    if (mode == 0) kfvo::mapKFUsingIDK(kfs[0], kfs[1].edges(), kfs[1].Pose, kfs[1].Pos, args[0], args[1], args[2]);
    else if (mode == 1) head[0] = kfvo::translateDepth_F2KF(kfs[0], kfs[1].edges(), kfs[1].Pose, kfs[1].Pos, kfs[1].K, flag != 0);
    else if (mode == 2) head[0] = kfvo::translateDepth_KF2F(kfs[0], kfs[1].edges(), kfs[1].Pose, kfs[1].Pos, kfs[1].K);
    else kfvo::translateDepth_New2Old(kfs, flag);
    res[1] = now() - t0;
    res[0] = nkf > 0 ? kfs[0].K : 0.0;
    FILE *f = fopen(argv[1], "wb");
    if (!f) return 6;
    fwrite(head, 4, 2, f);
    fwrite(res, 8, 2, f);
    for (int m = 0; m < nkf; m++) fwrite(kfs[m].edges().kl, sizeof(KeyLine), (size_t)kns[m], f);
    fclose(f);
    return 0;
}
