// Driver of the reference's exhaustive cross-view ray check for tools/make_surface_ray_cross_golden.py and
// tools/surface_ray_cross_timing.py (build machine only, never shipped).
//
// Compiled together with the reference's src/visualizer/surface_integrator.cpp, src/visualizer/depth_filler.cpp and
// src/mtracklib/keyframe.cpp, in place, and linked against oracle/_ref/libreforacle.so.  It builds a key-frame list whose depth_filler
// grids, poses and scales are the given ones (no fill is run; a view without a grid is a key frame without a depth filler), sets every
// grid's `dist` as keyframe::initDepthFiller does, by computeDistance(Zeros) (keyframe.cpp:181), and runs a list of steps of
// SurfaceInt::checkDFRayCrossExaustive(target, hidder) (surface_integrator.cpp:70-116).
//
// argv[1] input : int32 w, h, bw, bh, nviews, nsteps; float ppx, ppy, zfx, zfy;
//                 per view: double Pose[9] (row-major), Pos[3], K; int32 has_grid; if has_grid: double rho[G], s_rho[G];
//                 per step: int32 start (0 keep the flags, 1 ResetVisibility on every view, 2 the flags that follow), n (-1: every ordered
//                 pair t != h of the list), n x (int32 target, int32 hidder); if start == 2: uint8 visibility[nviews][G]
// argv[2] output: per step: uint8 visibility[nviews][G] (0 for a view without a grid); double seconds of each step
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
    int32_t hdr[6];
    float cam_f[4];
    if (!rd(hdr, sizeof hdr) || !rd(cam_f, sizeof cam_f)) return 2;
    const int w = hdr[0], h = hdr[1], bw = hdr[2], bh = hdr[3], nviews = hdr[4], nsteps = hdr[5];
    cam_model::rad_tan_distortion kc = {0, 0, 0, 0, 0};
    Size2D sz = {w, h};
    cam_model cam({cam_f[0], cam_f[1]}, {cam_f[2], cam_f[3]}, kc, sz);
    const int G = (w / bw) * (h / bh);

    std::vector<keyframe> kf_list(nviews);
    std::vector<double> grid(2 * (size_t)G);
    for (int v = 0; v < nviews; v++) {
        keyframe &kf = kf_list[v];
        double pose[13];
        int32_t has;
        if (!rd(pose, sizeof pose) || !rd(&has, 4)) return 3;
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) kf.Pose(i, j) = pose[3 * i + j];
            kf.Pos[i] = pose[9 + i];
        }
        kf.K = pose[12];
        kf.camera = cam;
        if (!has) continue;
        if (!rd(grid.data(), 16 * (size_t)G)) return 3;
        kf.df = std::shared_ptr<depth_filler>(new depth_filler(cam, {bw, bh}, depth_filler::BOUND_NONE));   // ResetData: visibility
        depth_filler &df = kf.depthFill();
        if (df.gridSize().w * df.gridSize().h != G) return 4;
        for (int i = 0; i < G; i++) {
            df.data[i].rho = grid[i];
            df.data[i].s_rho = grid[G + i];
        }
        df.computeDistance(TooN::Zeros);
    }

    FILE *fout = fopen(argv[2], "wb");
    if (!fout) return 6;
    std::vector<double> secs;
    std::vector<uint8_t> vis(G);
    for (int s = 0; s < nsteps; s++) {
        int32_t step[2];
        if (!rd(step, sizeof step)) return 7;
        std::vector<int32_t> ids(step[1] > 0 ? 2 * (size_t)step[1] : 0);
        if (!ids.empty() && !rd(ids.data(), 4 * ids.size())) return 8;
        for (size_t i = 0; i < ids.size(); i++)
            if (ids[i] < 0 || ids[i] >= nviews) return 9;
        if (step[0] == 1)
            for (keyframe &kf : kf_list)
                if (kf.depthFillerAval()) kf.depthFill().ResetVisibility();
        if (step[0] == 2)
            for (keyframe &kf : kf_list) {
                if (!rd(vis.data(), G)) return 10;
                if (kf.depthFillerAval())
                    for (int i = 0; i < G; i++) kf.depthFill().data[i].visibility = vis[i] != 0;
            }
        const double t0 = now();
        if (step[1] < 0) {
            for (int t = 0; t < nviews; t++)
                for (int hd = 0; hd < nviews; hd++)
                    if (t != hd) SurfaceInt::checkDFRayCrossExaustive(kf_list[t], kf_list[hd]);
        } else {
            for (size_t i = 0; i < ids.size(); i += 2) SurfaceInt::checkDFRayCrossExaustive(kf_list[ids[i]], kf_list[ids[i + 1]]);
        }
        secs.push_back(now() - t0);
        for (keyframe &kf : kf_list) {
            for (int i = 0; i < G; i++) vis[i] = kf.depthFillerAval() && kf.depthFill().data[i].visibility ? 1 : 0;
            fwrite(vis.data(), 1, G, fout);
        }
    }
    fwrite(secs.data(), 8, secs.size(), fout);
    fclose(fout);
    return 0;
}
