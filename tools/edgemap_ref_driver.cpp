// Driver of the reference's compressed edge map for tools/make_edgemap_golden.py (build machine only, never shipped).
//
// Compiled together with the reference's src/CommLib/edgemap_com.cpp, src/UtilLib/linefitting.cpp, src/UtilLib/libcrc.cpp and
// src/visualizer/depth_filler.cpp, in place, and linked against oracle/_ref/libreforacle.so for edge_finder.  It runs
//   edgemap_com_sender::compress_edgemap -> PreparePkg -> edgemap_com_decoder::Decode
// on one KeyLine list, and LineFitting::Fit2DLine<float, double> on the fit lists the generator names (the n_id path of n KeyLines from
// `start`, moved to homogeneous coordinates as RobustFit3DLine moves them), narrowed as RobustFit3DLine narrows them (linefitting.cpp:125-128).
//
// stdin : int32 kn, min_line_len, max_line_len, match_n_t, max_kl_num, nfit, w, h; double scale, max_angle, rho_rel_max;
//         float ppx, ppy, zfx, zfy; float nav[17]; kn x 168-byte KeyLines; nfit x {int32 start, n}
// stdout: int32 count; count x 5-byte records; int32 sent; int32 pkt_len; header + records of the packet; int32 nseg;
//         nseg x {float k0[4], k1[4]}; nfit x {float tx, ty, zfo}
// With an argument N (tools/edgemap_compress_timing.py): compress_edgemap runs N more times first and the mean wall time of a call, in
// milliseconds, goes to stderr.
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <vector>

#include "CommLib/edgemap_com.h"
#include "UtilLib/linefitting.h"

using namespace rebvo;

static bool rd(void *p, size_t n) { return fread(p, 1, n, stdin) == n; }
template <class T> static void wr(const T &v) { fwrite(&v, sizeof v, 1, stdout); }

int main(int argc, char **argv) {
    int32_t hdr[8];
    double dv[3];
    float fv[4], navf[17];
    if (!rd(hdr, sizeof hdr) || !rd(dv, sizeof dv) || !rd(fv, sizeof fv) || !rd(navf, sizeof navf)) return 2;
    const int kn = hdr[0], min_len = hdr[1], max_len = hdr[2], match_n_t = hdr[3], max_kl_num = hdr[4], nfit = hdr[5];
    static_assert(sizeof(KeyLine) == 168, "KeyLine layout");
    static_assert(sizeof(em_compressed_nav_pkg) == sizeof navf, "nav package layout");
    cam_model::rad_tan_distortion kc = {0, 0, 0, 0, 0};
    Size2D sz = {hdr[6], hdr[7]};
    cam_model cam({fv[0], fv[1]}, {fv[2], fv[3]}, kc, sz);
    static edge_finder ef(cam, 255 * 3);
    if (kn < 0 || kn + 1 > ef.kl_size) return 3;    // compress_edgemap's skip loop reads ef[kn] before it tests the bound
    memset(ef.kl, 0, sizeof(KeyLine) * (size_t)(kn + 1));
    if (kn > 0 && !rd(ef.kl, sizeof(KeyLine) * (size_t)kn)) return 4;
    ef.kn = kn;
    std::vector<int32_t> fits((size_t)nfit * 2 + 1);
    if (nfit > 0 && !rd(fits.data(), 8 * (size_t)nfit)) return 5;

    static edgemap_com_sender snd;
    if (argc > 1 && atoi(argv[1]) > 0) {
        const int reps = atoi(argv[1]);
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < reps; i++) snd.compress_edgemap(ef, dv[0], min_len, max_len, dv[1], cam, match_n_t, dv[2]);
        fprintf(stderr, "%.6f\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / reps);
        snd.edge_map_id = 0;
    }
    const int count = snd.compress_edgemap(ef, dv[0], min_len, max_len, dv[1], cam, match_n_t, dv[2]);
    wr((int32_t)count);
    for (int i = 0; i < count; i++) wr(snd[i]);

    em_compressed_nav_pkg nav;
    memcpy(&nav, navf, sizeof nav);
    const int sent = snd.PreparePkg(nav, max_kl_num);
    wr((int32_t)sent);
    const int32_t pkt_len = (int32_t)(snd.GetHdrSize() + snd.GetPkgSize());
    wr(pkt_len);
    fwrite(snd.GetHdrStr(), 1, snd.GetHdrSize(), stdout);
    fwrite(snd.GetPkgStr(), 1, snd.GetPkgSize(), stdout);

    static edgemap_com_decoder dec;
    const int nseg = dec.Decode(snd);
    wr((int32_t)nseg);
    for (int i = 0; i < nseg; i++) { wr(dec[i].k0); wr(dec[i].k1); }

    for (int f = 0; f < nfit; f++) {
        const int n = fits[2 * f + 1];
        std::vector<PPoint3D<float>> pl(n > 0 ? n : 1);
        int k = fits[2 * f];
        for (int i = 0; i < n; i++) {
            cam.Img2Hom(pl[i].x, pl[i].y, ef[k].c_p.x, ef[k].c_p.y);
            if (i < n - 1) k = ef[k].n_id;
        }
        Line2Dequ<double> equ2d;
        LineFitting::Fit2DLine(pl.data(), n, equ2d);
        float tx = equ2d.m2;
        float ty = -equ2d.m1;
        float zfo = sqrt(cam.zfm * cam.zfm + equ2d.m3 * equ2d.m3);
        wr(tx); wr(ty); wr(zfo);
    }
    return 0;
}
