// Driver of the reference's surface integrator for tools/make_surface_integrate_golden.py and tools/surface_integrate_timing.py (build
// machine only, never shipped).
//
// Compiled together with the reference's src/visualizer/surface_integrator.cpp, src/visualizer/depth_filler.cpp and
// src/mtracklib/keyframe.cpp, in place, and linked against oracle/_ref/libreforacle.so.  It builds a key-frame list whose depth_filler
// grids, poses and scales are the given ones (no fill is run), then what app/kf_visualizer/main.cpp does with it: analizeSpaceSize
// (:110), OcGrid with the explicit origin and size (:113), fillKFList (:116), and a list of ray cuts (:192 all key frames, :201 one).
// The reference prints to stdout (its "Out of size" messages among others), so the results go to the file named by argv[2].
//
// argv[1] input : int32 w, h, bw, bh, nviews, nx, ny, nz, ncuts; float ppx, ppy, zfx, zfy; double origin[3], size[3];
//                 per view: double Pose[9] (row-major), Pos[3], K, rho[G], s_rho[G];
//                 per cut: int32 reset (ResetVisibility on every view first), n (-1: rayCutSurface(kf_list)), n x int32 view ids
// argv[2] output: double space_origin[3], space_size[3] (analizeSpaceSize); uint32 blocks_filled; per cut: uint8 visibility[nviews][G];
//                 double seconds of fillKFList, then of each cut
#include <chrono>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>

#include "visualizer/surface_integrator.h"

using namespace rebvo;

static FILE *fin;
static bool rd(void *p, size_t n) { return fread(p, 1, n, fin) == n; }
static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char **argv) {
    if (argc < 3 || !(fin = fopen(argv[1], "rb"))) return 1;
    int32_t hdr[9];
    float cam_f[4];
    double box[6];
    if (!rd(hdr, sizeof hdr) || !rd(cam_f, sizeof cam_f) || !rd(box, sizeof box)) return 2;
    const int w = hdr[0], h = hdr[1], bw = hdr[2], bh = hdr[3], nviews = hdr[4], ncuts = hdr[8];
    cam_model::rad_tan_distortion kc = {0, 0, 0, 0, 0};
    Size2D sz = {w, h};
    cam_model cam({cam_f[0], cam_f[1]}, {cam_f[2], cam_f[3]}, kc, sz);
    const int G = (w / bw) * (h / bh);

    std::vector<keyframe> kf_list(nviews);
    std::vector<double> grid(2 * (size_t)G);
    for (int v = 0; v < nviews; v++) {
        keyframe &kf = kf_list[v];
        double pose[13];
        if (!rd(pose, sizeof pose) || !rd(grid.data(), 16 * (size_t)G)) return 3;
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) kf.Pose(i, j) = pose[3 * i + j];
            kf.Pos[i] = pose[9 + i];
        }
        kf.K = pose[12];
        kf.camera = cam;
        kf.df = std::shared_ptr<depth_filler>(new depth_filler(cam, {bw, bh}, depth_filler::BOUND_NONE));   // ResetData: visibility, father
        depth_filler &df = kf.depthFill();
        if (df.gridSize().w * df.gridSize().h != G) return 4;
        for (int i = 0; i < G; i++) {
            df.data[i].rho = grid[i];
            df.data[i].s_rho = grid[G + i];
        }
    }
    for (int v = 0; v < nviews; v++)     // hideAll tells the views apart by df_point::father
        for (int u = 0; u < v; u++)
            if (kf_list[v].depthFill().data[0].father == kf_list[u].depthFill().data[0].father) return 5;

    FILE *fout = fopen(argv[2], "wb");
    if (!fout) return 6;
    TooN::Vector<3> s_orig;
    TooN::Vector<3> s_size = SurfaceInt::analizeSpaceSize(kf_list, &s_orig);
    for (int i = 0; i < 3; i++) fwrite(&s_orig[i], 8, 1, fout);
    for (int i = 0; i < 3; i++) fwrite(&s_size[i], 8, 1, fout);

    std::vector<double> secs;
    OcGrid ocgrid(TooN::makeVector(box[0], box[1], box[2]), TooN::makeVector(box[3], box[4], box[5]),
                  {(u_int)hdr[5], (u_int)hdr[6], (u_int)hdr[7]});
    double t0 = now();
    const uint32_t filled = ocgrid.fillKFList(kf_list);
    secs.push_back(now() - t0);
    fwrite(&filled, 4, 1, fout);

    std::vector<uint8_t> vis(G);
    for (int c = 0; c < ncuts; c++) {
        int32_t cut[2];
        if (!rd(cut, sizeof cut)) return 7;
        std::vector<int32_t> ids(cut[1] > 0 ? cut[1] : 0);
        if (!ids.empty() && !rd(ids.data(), 4 * ids.size())) return 8;
        if (cut[0])
            for (keyframe &kf : kf_list) kf.depthFill().ResetVisibility();
        t0 = now();
        if (cut[1] < 0) {
            ocgrid.rayCutSurface(kf_list);
        } else {
            for (int32_t id : ids) {
                if (id < 0 || id >= nviews) return 9;
                ocgrid.rayCutSurface(kf_list[id]);
            }
        }
        secs.push_back(now() - t0);
        for (keyframe &kf : kf_list) {
            for (int i = 0; i < G; i++) vis[i] = kf.depthFill().data[i].visibility ? 1 : 0;
            fwrite(vis.data(), 1, G, fout);
        }
    }
    fwrite(secs.data(), 8, secs.size(), fout);
    fclose(fout);
    return 0;
}
