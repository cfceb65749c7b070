// Driver of the reference's key-frame match repair for tools/make_keyframe_track_golden.py (build machine only, never shipped).
//
// Compiled into a temporary directory outside the repository, together with the reference's src/mtracklib/keyframe.cpp and
// src/visualizer/depth_filler.cpp, in place (class keyframe's constructor lives there); the reference's src/mtracklib/kfvo.cpp is
// #included below (the functions under test); everything else comes from oracle/_ref/libreforacle.so.  kfvo.cpp's header chain (kfvo.h ->
// keyframe.h -> visualizer/depth_filler.h) needs std::max(float, double), which this image's C++ library does not resolve on its own: the
// generator pre-includes a header that declares it, as tools/make_depth_fill_golden.py does.  (oracle/ref_harness.cpp takes the header's
// include guard and declares a stand-in class instead; that works where no keyframe is constructed.)
//
// It runs what SecondThread runs per frame pair with TrackKeyFrames (rebvo_second_t.cpp:432-442):
//   kfvo::buildForwardMatch(kf, new, old); kfvo::forwardCorrectAugmentate(kf, new, Pose, Pos, thresh, tol, aug);
//   kfvo::correctAugmentate(kf, new, Pose, Pos, thresh, tol, aug)
//
// stdin : int32 kf_kn, new_kn, old_kn, augmentate; float zf; double dist_thresh, dist_tolerance, kf_Pose[9], kf_Pos[3], Pose[9], Pos[3];
//         kf_kn x 168-byte KeyLine records (the key frame's list), new_kn x 168-byte records (the new list)
// stdout: int32 fow_m0, fow_m, back_m, pad; double seconds[3]; int32 m_id_f after step 1 [kf_kn], after step 2 [kf_kn];
//         int32 m_id_kf of the new list after step 3 [new_kn]
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mtracklib/edge_tracker.h"
#include "mtracklib/global_tracker.h"
#include "src/mtracklib/kfvo.cpp"

using namespace rebvo;
using namespace TooN;

static bool rd(void *p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main() {
    int32_t hdr[4];
    float zf;
    double d[2 + 9 + 3 + 9 + 3];
    if (!rd(hdr, sizeof hdr) || !rd(&zf, 4) || !rd(d, sizeof d)) return 2;
    const int kf_kn = hdr[0], new_kn = hdr[1], old_kn = hdr[2];
    const bool aug = hdr[3] != 0;
    static_assert(sizeof(KeyLine) == 168, "KeyLine layout");
    cam_model::rad_tan_distortion kc = {0, 0, 0, 0, 0};
    Size2D sz = {752, 480};
    cam_model cam({376.f, 240.f}, {zf, zf}, kc, sz);
    edge_tracker et_kf(cam, 255 * 3), et_new(cam, 255 * 3), et_old(cam, 255 * 3);
    if (kf_kn > et_kf.kl_size || new_kn > et_new.kl_size || old_kn > et_old.kl_size) return 3;
    if (!rd(et_kf.kl, sizeof(KeyLine) * (size_t)kf_kn) || !rd(et_new.kl, sizeof(KeyLine) * (size_t)new_kn)) return 4;
    et_kf.kn = kf_kn; et_new.kn = new_kn; et_old.kn = old_kn;

    Matrix<3, 3> kfPose, Pose;
    Vector<3> kfPos, Pos;
    for (int i = 0; i < 9; i++) { kfPose(i / 3, i % 3) = d[2 + i]; Pose(i / 3, i % 3) = d[14 + i]; }
    for (int i = 0; i < 3; i++) { kfPos[i] = d[11 + i]; Pos[i] = d[23 + i]; }
    keyframe kf(et_kf, 0.0, 1.0, Identity, Zeros, Zeros, kfPose, Zeros, kfPos);

    int32_t cnt[4] = {0, 0, 0, 0};
    double sec[3];
    std::vector<int32_t> f0(kf_kn), f1(kf_kn), b1(new_kn);
    double t0 = now();
    cnt[0] = kfvo::buildForwardMatch(kf, et_new, et_old);
    sec[0] = now() - t0;
    for (int i = 0; i < kf_kn; i++) f0[i] = kf.edges()[i].m_id_f;
    t0 = now();
    cnt[1] = kfvo::forwardCorrectAugmentate(kf, et_new, Pose, Pos, d[0], d[1], aug);
    sec[1] = now() - t0;
    for (int i = 0; i < kf_kn; i++) f1[i] = kf.edges()[i].m_id_f;
    t0 = now();
    cnt[2] = kfvo::correctAugmentate(kf, et_new, Pose, Pos, d[0], d[1], aug);
    sec[2] = now() - t0;
    for (int i = 0; i < new_kn; i++) b1[i] = et_new[i].m_id_kf;

    fwrite(cnt, 4, 4, stdout);
    fwrite(sec, 8, 3, stdout);
    fwrite(f0.data(), 4, f0.size(), stdout);
    fwrite(f1.data(), 4, f1.size(), stdout);
    fwrite(b1.data(), 4, b1.size(), stdout);
    return 0;
}
