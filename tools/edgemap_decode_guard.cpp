// Stand-alone guard of the segment source of the depth fill, on the host: the steps the device takes — gates and step counts per
// segment, the scan of the counts, an item's segment by bisection of the offsets, its cell, the count / scan / stable scatter into cell
// buckets and the fold of each bucket in order — on random record lists, every index checked (std::vector::at), and the result compared
// with the serial fill_depth_map of rebvo/edgemap_com.h bit for bit.  Built with -fsanitize=address,undefined by
// tests/test_edgemap_decode_cpu.py; it has its own main and loads nothing.
//
// usage: edgemap_decode_guard [lists]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "rebvo/edgemap_com.h"

using namespace rebvo::edgemap;

static int seg_of(const std::vector<int> &off, int nseg, int i) {   // df_seg_of (depth_fill.hip)
    int lo = 0, hi = nseg;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off.at(mid) <= i) lo = mid; else hi = mid;
    }
    return lo;
}

int main(int argc, char **argv) {
    const int lists = argc > 1 ? atoi(argv[1]) : 200;
    std::mt19937 rng(12345);
    long long items_total = 0, segs_total = 0, over = 0;
    for (int l = 0; l < lists; l++) {
        const int w = 16 + (int)(rng() % 300), h = 16 + (int)(rng() % 200), bw = 1 + (int)(rng() % 12), bh = 1 + (int)(rng() % 12);
        if (w / bw < 1 || h / bh < 1) continue;
        const Camera cam = {(float)(w / 2.0 + (int)(rng() % 7) - 3), (float)(h / 2.0), 40.0 + (double)(rng() % 200), w, h};
        const int n = (int)(rng() % 60);
        std::vector<compressed_kl> rec((size_t)n + 1);
        for (int i = 0; i < n; i++) {
            const unsigned r = rng();
            rec[i].x = (uint8_t)(rng() % 256);
            rec[i].y = (uint8_t)(rng() % 256);
            rec[i].rho = (r % 5 == 0) ? 0 : (int16_t)((r % 3 == 0 ? -1 : 1) * (1 + (int)(rng() % 32767)));
            rec[i].s_rho = (uint8_t)(rng() % 7 == 0 ? (rng() % 2 ? 0 : 255) : rng() % 40);
        }
        const float rho_scale = 0.25f + (float)(rng() % 1000) / 100.f;
        const double v_thresh = (double)(rng() % 40) / 10.0, a_thresh = 20.0 + (double)(rng() % 70);
        const int cap_segments = 1 + (int)(rng() % 40), cap_items = (int)(rng() % 4000);
        std::vector<uncompressed_segment> walk, segs;
        decode(rec.data(), n, rho_scale, &walk, cap_segments);
        const int nseg = decode_local(rec.data(), n, rho_scale, &segs, cap_segments);
        if (walk.size() != segs.size()) { printf("list %d: decode differs\n", l); return 1; }
        for (int j = 0; j < nseg; j++)
            if (memcmp(&walk[j].k0, &segs[j].k0, 16) || memcmp(&walk[j].k1, &segs[j].k1, 16)) { printf("list %d: segment %d differs\n", l, j); return 1; }
        for (int j = 0; j < nseg; j++) segs[j].visi_mask = rng() % 3 != 0;
        const bool use_vis = rng() % 2;
        segs_total += nseg;

        // k_em_items: counts clamped to cap_items + 1, saturating scan
        const double cos_a = cos(a_thresh * M_PI / 180.0);
        const SegCam sc = cam.seg();
        const int sat = cap_items + 1;
        std::vector<int> off((size_t)nseg + 1, 0);
        std::vector<SegSteps> st((size_t)nseg);
        int run = 0;
        for (int j = 0; j < nseg; j++) {
            int steps = 0;
            if (!use_vis || segs.at(j).visi_mask) {
                st.at(j) = seg_steps(as_point(segs[j].k0), as_point(segs[j].k1), sc, v_thresh, cos_a, nullptr);
                steps = st[j].n < sat ? st[j].n : sat;
            }
            off.at(j) = run;
            run = run + steps < sat ? run + steps : sat;
        }
        off.at(nseg) = run;
        const bool overflow = run > cap_items;
        const int kn = overflow ? 0 : run;
        over += overflow;
        items_total += kn;

        // k_depth_fill<kDfSeg>: cells, counts, offsets, stable scatter, fold
        DepthGrid g(w, h, bw, bh);
        const int G = g.gw * g.gh;
        std::vector<int> cell((size_t)cap_items, -1), ids((size_t)cap_items, -1), cnt((size_t)G, 0), coff((size_t)G + 1, 0);
        for (int i = 0; i < kn; i++) {
            const int s = seg_of(off, nseg, i);
            if (!(off.at(s) <= i && i < off.at(s + 1))) { printf("list %d: item %d not in segment %d\n", l, i, s); return 1; }
            const int c = seg_step_cell(st.at(s), i - off.at(s), bw, bh, g.gw, g.gh);
            cell.at(i) = c;
            cnt.at(c)++;
        }
        for (int c = 0; c < G; c++) coff.at(c + 1) = coff.at(c) + cnt.at(c);
        std::vector<int> next(coff.begin(), coff.end() - 1);
        for (int i = 0; i < kn; i++) ids.at(next.at(cell.at(i))++) = i;
        for (int c = 0; c < G; c++) {
            for (int j = coff.at(c); j < coff.at(c + 1); j++) {
                const int i = ids.at(j), s = seg_of(off, nseg, i);
                seg_fold(seg_step_rho(st.at(s), i - off.at(s)), st.at(s).kl_I, &g.rho.at(c), &g.s_rho.at(c), &g.I_rho.at(c));
                g.fixed.at(c) = 1;
            }
        }
        DepthGrid ref(w, h, bw, bh);
        if (!overflow) {
            const long long steps = fill_depth_map(segs.data(), nseg, &ref, cam, v_thresh, a_thresh, use_vis);
            if (steps != kn) { printf("list %d: %lld steps, %d items\n", l, steps, kn); return 1; }
        }
        if (memcmp(g.rho.data(), ref.rho.data(), 8 * (size_t)G) || memcmp(g.s_rho.data(), ref.s_rho.data(), 8 * (size_t)G) ||
            memcmp(g.fixed.data(), ref.fixed.data(), (size_t)G)) { printf("list %d: grids differ\n", l); return 1; }
    }
    printf("ok: %d lists, %lld segments, %lld items, %lld over cap_items\n", lists, segs_total, items_total, over);
    return 0;
}
