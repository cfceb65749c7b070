// Driver of the reference's edgemap_com_decoder for tools/make_edgemap_decode_golden.py (build machine only, never shipped).
//
// Compiled together with the reference's src/CommLib/edgemap_com.cpp, src/UtilLib/linefitting.cpp, src/UtilLib/libcrc.cpp and
// src/visualizer/depth_filler.cpp, in place, and linked against oracle/_ref/libreforacle.so.  On one record list it runs
//   Decode -> per view {UpdatePos, GetDPose / GetDPos, HideVisible} -> ResetData -> fillDepthMap -> InitCoarseFine -> Integrate(iter_num)
// by calling the reference's own methods; nothing of their bodies is restated here.
//
// stdin : as tools/edgemap_decode_host_check.cpp reads it (use_visibility, zfm and the scalings are the host tool's: the reference has none)
// stdout: int32 nseg; nseg x {float k0[4], k1[4]}; per view {double DPose[9], DPos[3]; uint8 flags[nseg]; int32 s_num};
//         double rho[G], s_rho[G]; uint8 fixed[G] after fillDepthMap alone; the same three after the whole chain
// With reps > 0 (tools/edgemap_decode_timing.py): Decode, HideVisible of the first view and the fill chain run reps more times first and
// their mean wall times, in milliseconds, go to stderr.
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <chrono>
#include <vector>

#include "CommLib/edgemap_com.h"

using namespace rebvo;

static bool rd(void *p, size_t n) { return fread(p, 1, n, stdin) == n; }
template <class T> static void wr(const T &v) { fwrite(&v, sizeof v, 1, stdout); }

static void dump(depth_filler &df) {
    const Size2D g = df.gridSize();
    const size_t n = (size_t)g.w * g.h;
    std::vector<double> rho(n), s_rho(n);
    std::vector<uint8_t> fixed(n);
    for (size_t i = 0; i < n; i++) {
        rho[i] = df.data[i].rho;
        s_rho[i] = df.data[i].s_rho;
        fixed[i] = df.data[i].fixed ? 1 : 0;
    }
    fwrite(rho.data(), 8, n, stdout);
    fwrite(s_rho.data(), 8, n, stdout);
    fwrite(fixed.data(), 1, n, stdout);
}

int main() {
    int32_t hdr[10];
    float fv[5];
    double dv[5];
    static_assert(sizeof(em_compressed_nav_pkg) == 68, "nav package layout");
    static_assert(sizeof(compressed_kl) == 5, "record layout");
    em_compressed_nav_pkg em_nav;
    if (!rd(hdr, sizeof hdr) || !rd(fv, sizeof fv) || !rd(dv, sizeof dv) || !rd(&em_nav, sizeof em_nav)) return 2;
    const int n = hdr[0], w = hdr[1], h = hdr[2], bw = hdr[3], bh = hdr[4], iter_num = hdr[5], mode = hdr[6], nviews = hdr[7], reps = hdr[9];
    if (n < 0 || n > KEYLINE_MAX || nviews < 0) return 3;
    std::vector<em_compressed_nav_pkg> views((size_t)nviews + 1);
    if (nviews > 0 && !rd(views.data(), sizeof(em_compressed_nav_pkg) * (size_t)nviews)) return 4;
    static edgemap_com_decoder dec;
    if (n > 0 && !rd(dec.kls, sizeof(compressed_kl) * (size_t)n)) return 5;
    dec.kl_num = n;
    dec.rho_scale = fv[0];
    dec.em_pos = em_nav;
    cam_model::rad_tan_distortion kc = {0, 0, 0, 0, 0};
    Size2D sz = {(u_int)w, (u_int)h};
    cam_model cam({fv[1], fv[2]}, {fv[3], fv[4]}, kc, sz);
    depth_filler df(cam, {(u_int)bw, (u_int)bh}, (depth_filler::bound_modes)mode);

    if (reps > 0) {
        typedef std::chrono::steady_clock clk;
        auto ms = [&](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count() / reps; };
        auto t0 = clk::now();
        for (int i = 0; i < reps; i++) dec.Decode();
        const double t_dec = ms(t0);
        double t_hide = 0;
        if (nviews > 0) {
            t0 = clk::now();
            for (int i = 0; i < reps; i++) {
                for (int j = 0; j < dec.SegSize(); j++) dec[j].visi_mask = true;
                dec.HideVisible(views[0], cam);
            }
            t_hide = ms(t0);
        }
        t0 = clk::now();
        for (int i = 0; i < reps; i++) { df.ResetData(); dec.fillDepthMap(df, cam, dv[1], dv[2]); }
        const double t_fill = ms(t0);
        t0 = clk::now();
        for (int i = 0; i < reps; i++) { df.ResetData(); dec.fillDepthMap(df, cam, dv[1], dv[2]); df.InitCoarseFine(); df.Integrate(iter_num); }
        const double t_chain = ms(t0);
        fprintf(stderr, "%.6f %.6f %.6f %.6f\n", t_dec, t_hide, t_fill, t_chain);
    }

    const int nseg = dec.Decode();
    wr((int32_t)nseg);
    for (int i = 0; i < nseg; i++) { wr(dec[i].k0); wr(dec[i].k1); }
    for (int v = 0; v < nviews; v++) {
        dec.UpdatePos(views[v]);
        const TooN::Matrix<3, 3> R = dec.GetDPose();
        const TooN::Vector<3> P = dec.GetDPos();
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) wr((double)R[r][c]);
        for (int r = 0; r < 3; r++) wr((double)P[r]);
        const int s_num = dec.HideVisible(views[v], cam);
        for (int i = 0; i < nseg; i++) wr((uint8_t)(dec[i].visi_mask ? 1 : 0));
        wr((int32_t)s_num);
    }
    df.ResetData();
    dec.fillDepthMap(df, cam, dv[1], dv[2]);
    dump(df);
    df.InitCoarseFine();
    df.Integrate(iter_num);
    dump(df);
    return 0;
}
