// The host restatement of the compressed edge map (rebvo/edgemap_com.h) on one KeyLine list, for tests/edgemap_crafted.py: the CPU tests
// and tools/make_edgemap_golden.py compare its output with the compiled reference's (tools/edgemap_ref_driver.cpp).
//
// stdin : int32 kn, min_line_len, max_line_len, match_n_t, max_kl_num, cap; double scale, max_angle, rho_rel_max, x_scaling, y_scaling, zfm;
//         float ppx, ppy; float nav[17]; kn x 168-byte KeyLines
// stdout: int32 count, status; count x 5-byte records; int32 sent, pkt_len; the packet; int32 nseg; nseg x {float k0[4], k1[4]};
//         int32 nfit; nfit x {int32 start, n; float tx, ty, zfo; int32 flags}
// With the argument `recv`, the receiving side instead (Receiver::check_recv_pak on a fresh receiver, packet after packet):
// stdin : int32 keyline_max, npkt; npkt x {int32 brecv, len; len bytes}
// stdout: npkt x {int32 accepted, ready}; int32 kl_num, edge_map_id; float rho_scale; kl_num x 5-byte records
#include <cstdio>
#include <cstdint>
#include <string>
#include <vector>

#include "rebvo/edgemap_com.h"

using namespace rebvo::edgemap;

static bool rd(void *p, size_t n) { return fread(p, 1, n, stdin) == n; }
template <class T> static void wr(const T &v) { fwrite(&v, sizeof v, 1, stdout); }

static int recv_main() {
    int32_t h[2];
    if (!rd(h, sizeof h) || h[0] < 0) return 2;
    Receiver r(h[0]);
    for (int i = 0; i < h[1]; i++) {
        int32_t q[2];
        if (!rd(q, sizeof q) || q[1] < 0) return 3;
        std::vector<uint8_t> pkt((size_t)q[1] + 1);
        if (q[1] > 0 && !rd(pkt.data(), (size_t)q[1])) return 4;
        bool ready = false;
        const bool ok = r.check_recv_pak(pkt.data(), q[0] <= q[1] ? q[0] : q[1], &ready);
        wr((int32_t)ok); wr((int32_t)ready);
    }
    wr((int32_t)r.em.kl_num); wr((int32_t)r.em.edge_map_id); wr(r.em.rho_scale);
    fwrite(r.em.kls.data(), sizeof(compressed_kl), (size_t)r.em.kl_num, stdout);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && std::string(argv[1]) == "recv") return recv_main();
    int32_t hdr[6];
    double dv[6];
    float pp[2];
    em_compressed_nav_pkg nav;
    if (!rd(hdr, sizeof hdr) || !rd(dv, sizeof dv) || !rd(pp, sizeof pp) || !rd(&nav, sizeof nav)) return 2;
    const int kn = hdr[0], cap = hdr[5];
    if (kn < 0 || cap < 0) return 3;
    std::vector<edgehip_keyline> kl((size_t)kn + 1);
    if (kn > 0 && !rd(kl.data(), sizeof(edgehip_keyline) * (size_t)kn)) return 4;
    edgehip_edgemap_params p = {};
    p.min_line_len = hdr[1]; p.max_line_len = hdr[2]; p.match_n_t = hdr[3];
    p.max_angle = dv[1]; p.rho_rel_max = dv[2]; p.x_scaling = dv[3]; p.y_scaling = dv[4];
    std::vector<compressed_kl> rec((size_t)cap + 1);
    std::vector<FitTrace> trace(4 * (size_t)kn + 8);
    int status = 0, nfit = 0;
    const int count = rebvo_compress_edgemap(kl.data(), kn, p, dv[0], pp[0], pp[1], dv[5], rec.data(), cap, &status, trace.data(), &nfit);
    if (count < 0) return 5;
    wr((int32_t)count); wr((int32_t)status);
    fwrite(rec.data(), sizeof(compressed_kl), (size_t)count, stdout);

    std::vector<uint8_t> pkt;
    int sr = 0;
    const int sent = prepare_pkg(rec.data(), count, &sr, 1, (float)dv[0], nav, hdr[4], &pkt);
    if (sent < 0) return 6;
    wr((int32_t)sent); wr((int32_t)pkt.size());
    fwrite(pkt.data(), 1, pkt.size(), stdout);

    std::vector<uncompressed_segment> segs;
    const int nseg = decode(rec.data(), count, (float)dv[0], &segs, 50000, p.x_scaling == 0 ? 0.5 : p.x_scaling, p.y_scaling == 0 ? 1.0 : p.y_scaling);
    wr((int32_t)nseg);
    for (const auto &s : segs) { wr(s.k0); wr(s.k1); }
    wr((int32_t)nfit);
    for (int i = 0; i < nfit; i++) wr(trace[i]);
    return 0;
}
