// Driver of the reference's depth_filler surface for tools/make_depth_surface_golden.py (build machine only, never shipped).
//
// Compiled together with the reference's src/visualizer/depth_filler.cpp, in place, and linked against oracle/_ref/libreforacle.so
// for edge_tracker.  It runs the fill as tools/depth_fill_ref_driver.cpp does, then what the reference's callers take from the grid:
//   computeDistance(Zeros) (visualizer.cpp:436-440, keyframe.cpp:181), get3DPos per cell, calcSurfNormals, calcSurfArea, and
//   getImgRho / getImgRhoTriInterp with s_rho at the requested pixels.
// Before calcSurfNormals / calcSurfArea every cell's normal and area are set to a NaN sentinel, so the output shows which cells the
// reference never writes.
//
// stdin : int32 w, h, bw, bh, iter_num, bound_mode, discard, m_num_t; double v_thresh; float ppx, ppy, zfx, zfy;
//         int32 kn; kn x 168-byte KeyLine records; int32 np; np x (int32 px, int32 py)
// stdout: double point[G][3], dist[G], min_dist, normal[G][3]; float area[G];
//         double rho1[np], s_rho1[np] (getImgRho), rho2[np], s_rho2[np] (getImgRhoTriInterp)
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>

#include "visualizer/depth_filler.h"

using namespace rebvo;

static bool rd(void *p, size_t n) { return fread(p, 1, n, stdin) == n; }

static const uint64_t kSentinel64 = 0x7FF4DEADBEEF0001ull;
static const uint32_t kSentinel32 = 0x7FA0DEADu;

int main() {
    int32_t hdr[8];
    double v_thresh;
    float cam_f[4];
    int32_t kn;
    if (!rd(hdr, sizeof hdr) || !rd(&v_thresh, 8) || !rd(cam_f, sizeof cam_f) || !rd(&kn, 4)) return 2;
    const int w = hdr[0], h = hdr[1], bw = hdr[2], bh = hdr[3], iter_num = hdr[4], mode = hdr[5], discard = hdr[6], m_num_t = hdr[7];
    static_assert(sizeof(KeyLine) == 168, "KeyLine layout");
    cam_model::rad_tan_distortion kc = {0, 0, 0, 0, 0};
    Size2D sz = {w, h};
    cam_model cam({cam_f[0], cam_f[1]}, {cam_f[2], cam_f[3]}, kc, sz);
    edge_tracker et(cam, 255 * 3);
    if (kn > et.kl_size) return 3;
    if (kn > 0 && !rd(et.kl, sizeof(KeyLine) * (size_t)kn)) return 4;
    et.kn = kn;
    int32_t np;
    if (!rd(&np, 4) || np < 0) return 5;
    std::vector<int32_t> pix(2 * (size_t)np);
    if (np > 0 && !rd(pix.data(), 8 * (size_t)np)) return 6;

    depth_filler df(cam, {bw, bh}, (depth_filler::bound_modes)mode);
    df.ResetData();
    df.FillEdgeData(et, v_thresh, m_num_t, discard != 0);
    df.InitCoarseFine();
    df.Integrate(iter_num);
    df.computeDistance(TooN::Zeros);

    const Size2D g = df.gridSize();
    const int n = g.w * g.h;
    double s64;
    float s32;
    memcpy(&s64, &kSentinel64, 8);
    memcpy(&s32, &kSentinel32, 4);
    for (int i = 0; i < n; i++) {
        df.data[i].normal = TooN::makeVector(s64, s64, s64);
        df.data[i].area = s32;
    }
    df.calcSurfNormals();
    df.calcSurfArea();

    std::vector<double> point(3 * (size_t)n), dist(n), normal(3 * (size_t)n);
    std::vector<float> area(n);
    for (int y = 0; y < g.h; y++)
        for (int x = 0; x < g.w; x++) {
            const int i = y * g.w + x;
            const TooN::Vector<3> P = df.get3DPos(x, y);
            for (int k = 0; k < 3; k++) {
                point[3 * i + k] = P[k];
                normal[3 * i + k] = df.data[i].normal[k];
            }
            dist[i] = df.data[i].dist;
            area[i] = df.data[i].area;
        }
    const double min_dist = df.GetMinDist();
    std::vector<double> img(4 * (size_t)np);
    for (int j = 0; j < np; j++) {
        double s1 = 0, s2 = 0;
        img[j] = df.getImgRho(pix[2 * j], pix[2 * j + 1], &s1);
        img[np + j] = s1;
        img[2 * (size_t)np + j] = df.getImgRhoTriInterp(pix[2 * j], pix[2 * j + 1], &s2);
        img[3 * (size_t)np + j] = s2;
    }
    fwrite(point.data(), 8, point.size(), stdout);
    fwrite(dist.data(), 8, n, stdout);
    fwrite(&min_dist, 8, 1, stdout);
    fwrite(normal.data(), 8, normal.size(), stdout);
    fwrite(area.data(), 4, n, stdout);
    fwrite(img.data(), 8, img.size(), stdout);
    return 0;
}
