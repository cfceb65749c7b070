// Driver of the reference's depth_filler, net_keyline overload, for tools/make_depth_fill_net_golden.py (build machine only, never shipped).
//
// Compiled together with the reference's src/visualizer/depth_filler.cpp, in place, and linked against oracle/_ref/libreforacle.so.
// It runs the chain the reference's visualizer runs per received frame (visualizer.cpp:436-439):
//   ResetData -> FillEdgeData(net_keyline*, kn, p_off, v_thresh, m_num_t, discart) -> InitCoarseFine -> Integrate(iter_num)
// A record whose cell index lands past the grid makes the reference write past its buffer; the grid is given room behind its last cell
// for the largest index the records produce (Image::GetIndex on the reference's own expression), so those writes land there and the
// fixture's grid is what the cells inside hold: such records are dropped.
//
// stdin : int32 w, h, bw, bh, iter_num, bound_mode, discard, m_num_t; double v_thresh; float p_off_x, p_off_y; int32 kn; kn x 15-byte records
// stdout: double rho[gh*gw], double s_rho[gh*gw], uint8 fixed[gh*gw] (row-major)
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>

#include "visualizer/depth_filler.h"
#include "CommLib/net_keypoint.h"

using namespace rebvo;

static bool rd(void *p, size_t n) { return fread(p, 1, n, stdin) == n; }

int main() {
    int32_t hdr[8];
    double v_thresh;
    float p_off[2];
    int32_t kn;
    if (!rd(hdr, sizeof hdr) || !rd(&v_thresh, 8) || !rd(p_off, 8) || !rd(&kn, 4)) return 2;
    const int w = hdr[0], h = hdr[1], bw = hdr[2], bh = hdr[3], iter_num = hdr[4], mode = hdr[5], discard = hdr[6], m_num_t = hdr[7];
    static_assert(sizeof(net_keyline) == 15, "net_keyline layout");
    if (kn < 0 || kn > KEYLINE_MAX) return 3;
    std::vector<net_keyline> kl(kn > 0 ? kn : 1);
    if (kn > 0 && !rd(kl.data(), sizeof(net_keyline) * (size_t)kn)) return 4;
    cam_model::rad_tan_distortion kc = {0, 0, 0, 0, 0};
    Size2D sz = {(u_int)w, (u_int)h};
    cam_model cam({(float)(w / 2), (float)(h / 2)}, {(float)w, (float)w}, kc, sz);

    depth_filler df(cam, {(u_int)bw, (u_int)bh}, (depth_filler::bound_modes)mode);
    const Size2D g = df.gridSize();
    const size_t n = (size_t)g.w * g.h;
    Point2DF off = {p_off[0], p_off[1]};
    size_t top = n;
    for (int i = 0; i < kn; i++) {
        const size_t inx = df.data.GetIndex((kl[i].qx + off.x) / df.bl_size.w, (kl[i].qy + off.y) / df.bl_size.h);
        if (inx >= top) top = inx + 1;
    }
    if (top > 64 * n + 4096) return 5;   // an index that wrapped: not a fixture
    df_point *own = df.data.data;
    std::vector<df_point> room(top);
    df.data.data = room.data();
    df.ResetData();
    df.FillEdgeData(kl.data(), kn, off, v_thresh, m_num_t, discard != 0);
    df.InitCoarseFine();
    df.Integrate(iter_num);

    std::vector<double> rho(n), s_rho(n);
    std::vector<uint8_t> fixed(n);
    for (size_t i = 0; i < n; i++) {
        rho[i] = df.data[i].rho;
        s_rho[i] = df.data[i].s_rho;
        fixed[i] = df.data[i].fixed ? 1 : 0;
    }
    df.data.data = own;
    fwrite(rho.data(), 8, n, stdout);
    fwrite(s_rho.data(), 8, n, stdout);
    fwrite(fixed.data(), 1, n, stdout);
    return 0;
}
