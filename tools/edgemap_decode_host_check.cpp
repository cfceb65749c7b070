// The host restatement of the compressed edge map's receiving side (rebvo/edgemap_com.h: decode, update_pos, hide_visible,
// fill_depth_map) on one record list, for tests/edgemap_decode_crafted.py: the CPU tests and tools/make_edgemap_decode_golden.py compare
// its output with the compiled reference's (tools/edgemap_decode_ref_driver.cpp), which reads the same input.
//
// stdin : int32 n_rec, w, h, bw, bh, iter_num, bound_mode, nviews, use_visibility, reps; float rho_scale, ppx, ppy, zfx, zfy;
//         double zfm, v_thresh, a_thresh_deg, x_scaling, y_scaling; float em_nav[17]; nviews x float nav[17]; n_rec x 5-byte records
// stdout: int32 nseg; nseg x {float k0[4], k1[4]}; per view {double DPose[9], DPos[3]; uint8 flags[nseg]; int32 s_num};
//         double rho[G], s_rho[G]; uint8 fixed[G] after fill_depth_map alone; int32 gates[nseg]; int64 steps
// (iter_num, bound_mode, zfx, zfy and reps are the driver's.)  The fill runs after the views: with use_visibility it skips what they hid.
// Exit 9 when decode_local (the rule the device runs) differs from decode (the cursor walk).
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>

#include "rebvo/edgemap_com.h"

using namespace rebvo::edgemap;

static bool rd(void *p, size_t n) { return fread(p, 1, n, stdin) == n; }
template <class T> static void wr(const T &v) { fwrite(&v, sizeof v, 1, stdout); }

int main() {
    int32_t hdr[10];
    float fv[5];
    double dv[5];
    em_compressed_nav_pkg em_nav;
    if (!rd(hdr, sizeof hdr) || !rd(fv, sizeof fv) || !rd(dv, sizeof dv) || !rd(&em_nav, sizeof em_nav)) return 2;
    const int n = hdr[0], nviews = hdr[7];
    if (n < 0 || nviews < 0 || hdr[3] < 1 || hdr[4] < 1) return 3;
    std::vector<em_compressed_nav_pkg> views((size_t)nviews + 1);
    if (nviews > 0 && !rd(views.data(), sizeof(em_compressed_nav_pkg) * (size_t)nviews)) return 4;
    std::vector<compressed_kl> rec((size_t)n + 1);
    if (n > 0 && !rd(rec.data(), sizeof(compressed_kl) * (size_t)n)) return 5;
    const double xs = dv[3] == 0 ? 0.5 : dv[3], ys = dv[4] == 0 ? 1.0 : dv[4];
    const Camera cam = {fv[1], fv[2], dv[0], hdr[1], hdr[2]};

    std::vector<uncompressed_segment> segs, local;
    const int nseg = decode(rec.data(), n, fv[0], &segs, 1 << 30, xs, ys);
    decode_local(rec.data(), n, fv[0], &local, 1 << 30, xs, ys);
    if (local.size() != segs.size()) return 9;
    for (int i = 0; i < nseg; i++)
        if (memcmp(&local[i].k0, &segs[i].k0, sizeof(uncompressed_kl)) || memcmp(&local[i].k1, &segs[i].k1, sizeof(uncompressed_kl))) return 9;
    wr((int32_t)nseg);
    for (const auto &s : segs) { wr(s.k0); wr(s.k1); }

    for (int v = 0; v < nviews; v++) {
        const PosDelta d = update_pos(em_nav, views[v]);
        fwrite(d.DPose, 8, 9, stdout);
        fwrite(d.DPos, 8, 3, stdout);
        const int s_num = hide_visible(segs.data(), nseg, d, em_nav.K, views[v].K, cam);
        for (const auto &s : segs) wr((uint8_t)(s.visi_mask ? 1 : 0));
        wr((int32_t)s_num);
    }

    DepthGrid g(hdr[1], hdr[2], hdr[3], hdr[4]);
    std::vector<int32_t> gates((size_t)nseg + 1);
    const long long steps = fill_depth_map(segs.data(), nseg, &g, cam, dv[1], dv[2], hdr[8] != 0, gates.data());
    fwrite(g.rho.data(), 8, g.rho.size(), stdout);
    fwrite(g.s_rho.data(), 8, g.s_rho.size(), stdout);
    fwrite(g.fixed.data(), 1, g.fixed.size(), stdout);
    fwrite(gates.data(), 4, (size_t)nseg, stdout);
    wr((int64_t)steps);
    return 0;
}
