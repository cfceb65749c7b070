// Driver of the reference's depth_filler for tools/make_depth_fill_golden.py (build machine only, never shipped).
//
// Compiled together with the reference's src/visualizer/depth_filler.cpp, in place, and linked against oracle/_ref/libreforacle.so
// for edge_tracker.  It runs the chain both reference callers run (visualizer.cpp:436-440, keyframe.cpp:171-184):
//   ResetData -> FillEdgeData(edge_tracker&, v_thresh, m_num_t, discart) -> InitCoarseFine -> Integrate(iter_num)
//
// stdin : int32 w, h, bw, bh, iter_num, bound_mode, discard, m_num_t; double v_thresh; int32 kn; kn x 168-byte KeyLine records
// stdout: double rho[gh*gw], double s_rho[gh*gw], uint8 fixed[gh*gw] (row-major)
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>

#include "visualizer/depth_filler.h"

using namespace rebvo;

static bool rd(void *p, size_t n) { return fread(p, 1, n, stdin) == n; }

int main() {
    int32_t hdr[8];
    double v_thresh;
    int32_t kn;
    if (!rd(hdr, sizeof hdr) || !rd(&v_thresh, 8) || !rd(&kn, 4)) return 2;
    const int w = hdr[0], h = hdr[1], bw = hdr[2], bh = hdr[3], iter_num = hdr[4], mode = hdr[5], discard = hdr[6], m_num_t = hdr[7];
    static_assert(sizeof(KeyLine) == 168, "KeyLine layout");
    cam_model::rad_tan_distortion kc = {0, 0, 0, 0, 0};
    Size2D sz = {w, h};
    cam_model cam({(float)(w / 2), (float)(h / 2)}, {(float)w, (float)w}, kc, sz);
    edge_tracker et(cam, 255 * 3);
    if (kn > et.kl_size) return 3;
    if (kn > 0 && !rd(et.kl, sizeof(KeyLine) * (size_t)kn)) return 4;
    et.kn = kn;

    depth_filler df(cam, {bw, bh}, (depth_filler::bound_modes)mode);
    df.ResetData();
    df.FillEdgeData(et, v_thresh, m_num_t, discard != 0);
    df.InitCoarseFine();
    df.Integrate(iter_num);

    const Size2D g = df.gridSize();
    const int n = g.w * g.h;
    std::vector<double> rho(n), s_rho(n);
    std::vector<uint8_t> fixed(n);
    for (int i = 0; i < n; i++) {
        rho[i] = df.data[i].rho;
        s_rho[i] = df.data[i].s_rho;
        fixed[i] = df.data[i].fixed ? 1 : 0;
    }
    fwrite(rho.data(), 8, n, stdout);
    fwrite(s_rho.data(), 8, n, stdout);
    fwrite(fixed.data(), 1, n, stdout);
    return 0;
}
