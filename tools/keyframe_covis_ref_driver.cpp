// Driver of the reference's key-frame pair scoring for tools/make_keyframe_covis_golden.py and tools/keyframe_covis_timing.py (build
// machine only, never shipped).
//
// Compiled into a temporary directory outside the repository, together with the reference's src/mtracklib/keyframe.cpp and
// src/visualizer/depth_filler.cpp, in place; the reference's src/mtracklib/kfvo.cpp is #included below (the functions under test), and
// src/mtracklib/global_tracker.cpp comes with it the same way (build_field and the float instantiation of Calc_f_J_Complete live there);
// everything else comes from oracle/_ref/libreforacle.so, whose own copies of these symbols the program's definitions take precedence over.  The
// generator pre-includes a header that declares std::max(float, double), as tools/make_keyframe_track_golden.py does.
//
// It builds M keyframe objects from records, each one's field with global_tracker::build_field(edges, radius, min_mod), and runs
// kfvo::countMatches(kf_to, kf_from, ...) and kfvo::kls_on_fov(kf_from, kf_to.Pose, kf_to.Pos) on every ordered pair, on copies of the
// lists (countMatches writes m_id_f; nothing else).
//
// stdin : int32 M, w, h, radius; float min_mod, match_mod, match_ang, rho_tol, max_r, ppx, ppy, zfx, zfy;
//         per key frame: int32 kn, pad; double Pose[9], Pos[3], K; kn x 168-byte KeyLine records
// stdout: int32 sizeof(cos(match_ang)) as kfvo.cpp's call binds it, pad; double seconds[2] (fields, pairs);
//         int32 counts[M][M][3] (index [to][from]: kl_on_fov, kl_match, kls_on_fov); int32 field[M][h*w][2] (dist, ikl; dist 0 where empty)
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "mtracklib/edge_tracker.h"
#include "mtracklib/global_tracker.h"
#include "src/mtracklib/kfvo.cpp"
#include "src/mtracklib/global_tracker.cpp"

namespace rebvo {
// the width of the value kfvo.cpp:45's cos(match_ang) returns, in that file's own scope (namespace rebvo, using namespace TooN)
static int cos_width() { float a = 0.5f; return (int)sizeof(cos(a)); }
}

using namespace rebvo;
using namespace TooN;

static bool rd(void *p, size_t n) { return n == 0 || fread(p, 1, n, stdin) == n; }
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main() {
    int32_t hdr[4];
    float fl[9];
    if (!rd(hdr, sizeof hdr) || !rd(fl, sizeof fl)) return 2;
    const int M = hdr[0], w = hdr[1], h = hdr[2], radius = hdr[3];
    static_assert(sizeof(KeyLine) == 168, "KeyLine layout");
    cam_model::rad_tan_distortion kc = {0, 0, 0, 0, 0};
    Size2D sz = {(unsigned)w, (unsigned)h};
    cam_model cam({fl[5], fl[6]}, {fl[7], fl[8]}, kc, sz);
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
    double sec[2] = {0, 0};
    double t0 = now();
    for (keyframe &kf : kfs) kf.tracker().build_field(kf.edges(), radius, fl[0]);
    sec[0] = now() - t0;
    std::vector<int32_t> cnt((size_t)M * M * 3);
    t0 = now();
    for (int to = 0; to < M; to++)
        for (int from = 0; from < M; from++) {
            int on_fov = 0, match = 0;
            kfvo::countMatches(kfs[to], kfs[from], on_fov, match, fl[1], fl[2], fl[3], fl[4]);
            int32_t *c = &cnt[((size_t)to * M + from) * 3];
            c[0] = on_fov; c[1] = match;
            c[2] = kfvo::kls_on_fov(kfs[from], kfs[to].Pose, kfs[to].Pos);
        }
    sec[1] = now() - t0;
    int32_t head[2] = {cos_width(), 0};
    fwrite(head, 4, 2, stdout);
    fwrite(sec, 8, 2, stdout);
    fwrite(cnt.data(), 4, cnt.size(), stdout);
    std::vector<int32_t> f((size_t)w * h * 2);
    for (keyframe &kf : kfs) {
        global_tracker &g = kf.tracker();
        for (int i = 0; i < w * h; i++) {
            f[2 * i + 1] = g.field[i].ikl;
            f[2 * i] = g.field[i].ikl >= 0 ? g.field[i].dist : 0;
        }
        fwrite(f.data(), 4, f.size(), stdout);
    }
    return 0;
}
