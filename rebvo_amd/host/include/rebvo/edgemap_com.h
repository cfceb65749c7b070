// edgemap_com.h — the reference's compressed edge map on the host (include/CommLib/edgemap_com.h, src/CommLib/edgemap_com.cpp), header-only:
//   rebvo_compress_edgemap   edgemap_com_sender::compress_edgemap (:168-326) as the straight serial loop over an AoS KeyLine list, on
//                            the walk and the fit the device runs (csrc/edgemap_fit.h); what edgehip_edgemap_compress is tested against
//   compressed_kl, em_compressed_nav_pkg, compressed_edgemap_hdr   the wire structs (edgemap_com.h:45-102), packed
//   crc16                    util::CRC16 (src/UtilLib/libcrc.cpp): the reflected 0xA001 polynomial from 0xFFFF, table generated here
//   prepare_pkg              edgemap_com_sender::PreparePkg (:329-353): header with both CRC-16 fields + the records of one packet
//   Receiver::check_recv_pak edgemap_com_receiver::CheckRecvPak (:374-429)
//   get_pair / decode        edgemap_com::getPair (:46-86), edgemap_com_decoder::Decode (:431-440)
#pragma once
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <stdlib.h>
#include <vector>

#include "edgehip.h"
#include "edgemap_fit.h"

namespace rebvo {
namespace edgemap {

#pragma pack(push, 1)
struct compressed_kl {
    uint8_t x, y;
    int16_t rho;
    uint8_t s_rho;
};
struct em_compressed_nav_pkg {
    float p[3], w[3], g[3], ps[3];
    float K;
    float ref_err[4];
};
struct compressed_edgemap_hdr {
    uint16_t paket_size;
    uint16_t edgemap_id;
    float rho_scale;
    uint32_t kl_id, kl_num, kl_total;
    em_compressed_nav_pkg nav;
    uint16_t crc_em;
    uint16_t crc;
};
#pragma pack(pop)
static_assert(sizeof(compressed_kl) == 5 && sizeof(compressed_kl) == sizeof(edgehip_compressed_kl), "compressed_kl is 5 bytes");
static_assert(sizeof(em_compressed_nav_pkg) == 68, "em_compressed_nav_pkg is 17 floats");
static_assert(sizeof(compressed_edgemap_hdr) == 92, "compressed_edgemap_hdr is 92 bytes");

struct uncompressed_kl { float x, y, rho, s_rho; };   // PPoint3D<float>
struct uncompressed_segment {
    uncompressed_kl k0, k1;
    bool visi_mask;
};

// ---- the KeyLine list and the mask as edgemap_fit.h reads them ------------------------------------------------------------------------
struct AosKeyLines {
    const edgehip_keyline *kl;
    int n;
    int kn() const { return n; }
    int next(int k) const { return link_in_range(kl[k].n_id, n); }
    int prev(int k) const { return link_in_range(kl[k].p_id, n); }
    float cx(int k) const { return kl[k].c_p[0]; }
    float cy(int k) const { return kl[k].c_p[1]; }
    float ux(int k) const { return kl[k].u_m[0]; }
    float uy(int k) const { return kl[k].u_m[1]; }
    double rho(int k) const { return kl[k].rho; }
    double s_rho(int k) const { return kl[k].s_rho; }
    int m_num(int k) const { return kl[k].m_num; }
};
struct ByteMask {
    uint8_t *m;
    bool get(int k) const { return m[k] != 0; }
    void set(int k) { m[k] = 1; }
    void clear(int k) { m[k] = 0; }
};
struct SpanOut {     // records into a caller-given span; a record past its end is dropped (the caller sees count > cap)
    enum { kFit = 1 };
    compressed_kl *out;
    int base, cap;
    void put(int i, const Rec &r) {
        if (base + i < cap) { out[base + i].x = r.x; out[base + i].y = r.y; out[base + i].rho = r.rho; out[base + i].s_rho = r.s_rho; }
    }
};

inline WalkParams walk_params(const edgehip_edgemap_params &p, double scale, float ppx, float ppy, double zfm) {
    WalkParams w;
    w.min_line_len = p.min_line_len; w.max_line_len = p.max_line_len; w.match_n_t = p.match_n_t;
    w.max_cangle = cos(p.max_angle);
    w.rho_rel_max = p.rho_rel_max;
    w.x_scaling = p.x_scaling == 0 ? 0.5 : p.x_scaling;
    w.y_scaling = p.y_scaling == 0 ? 1.0 : p.y_scaling;
    w.scale = scale;
    w.ppx = ppx; w.ppy = ppy; w.zfm = zfm;
    return w;
}
inline bool params_ok(const edgehip_edgemap_params &p) {
    return p.min_line_len >= 0 && p.max_line_len >= 1 && p.x_scaling >= 0 && p.y_scaling >= 0;
}

// compress_edgemap over kl[kn] into out[cap].  Returns the number of records (0 with kOverflow in *status when they exceed cap, -1 for
// parameters the rule does not cover).  trace / ntrace: every fit's tx, ty, zfo in the order the fits run (room for kn + 1), or null.
inline int rebvo_compress_edgemap(const edgehip_keyline *kl, int kn, const edgehip_edgemap_params &p, double scale, float ppx, float ppy,
                                  double zfm, compressed_kl *out, int cap, int *status, FitTrace *trace = nullptr, int *ntrace = nullptr) {
    int st = 0, nt = 0;
    if (status) *status = 0;
    if (kn < 0 || cap < 0 || !params_ok(p)) return -1;
    const WalkParams w = walk_params(p, scale, ppx, ppy, zfm);
    const AosKeyLines acc = {kl, kn};
    std::vector<uint8_t> bits((size_t)kn + 1, 0);
    ByteMask mask = {bits.data()};
    for (int k = 0; k < kn; k++)
        if (link_is_bad(kl[k].n_id, kn) || link_is_bad(kl[k].p_id, kn)) st |= kBadLink;
    int c = 0;
    for (int k = 0; k < kn; k++) {
        if (mask.get(k) || acc.prev(k) >= 0) continue;
        SpanOut o = {out, c, cap};
        c += walk_head(acc, mask, w, k, o, st, trace, trace ? &nt : nullptr);
    }
    if (c > cap) { c = 0; st |= kOverflow; }
    if (status) *status = st;
    if (ntrace) *ntrace = nt;
    return c;
}

// ---- util::CRC16 ----------------------------------------------------------------------------------------------------------------------
inline uint16_t crc16(const uint8_t *msg, uint16_t len) {
    static uint16_t table[256];
    static bool ready = false;
    if (!ready) {
        for (int i = 0; i < 256; i++) {
            uint16_t c = (uint16_t)i;
            for (int b = 0; b < 8; b++) c = (c & 1) ? (uint16_t)((c >> 1) ^ 0xA001) : (uint16_t)(c >> 1);
            table[i] = c;
        }
        ready = true;
    }
    uint16_t crc = 0xFFFF;
    while (len--) crc = (uint16_t)((crc >> 8) ^ table[(crc ^ *msg++) & 0xFF]);
    return crc;
}

// ---- PreparePkg -----------------------------------------------------------------------------------------------------------------------
// One packet of the records [*sr_inx, *sr_inx + min(max_kl_num, kl_num - *sr_inx)): header, then the records.  paket_size and the CRC's
// length argument are 16-bit in the reference: a max_kl_num whose packet does not fit 65535 bytes is refused (-1, nothing written).
// Returns the records sent and advances *sr_inx.
inline int prepare_pkg(const compressed_kl *kls, int kl_num, int *sr_inx, uint16_t edgemap_id, float rho_scale, const em_compressed_nav_pkg &nav,
                       int max_kl_num, std::vector<uint8_t> *pkt) {
    if (max_kl_num < 0 || (size_t)max_kl_num * sizeof(compressed_kl) + sizeof(compressed_edgemap_hdr) > 65535u) return -1;
    if (kl_num < 0 || *sr_inx < 0 || *sr_inx > kl_num) return -1;
    const int to_send = max_kl_num < kl_num - *sr_inx ? max_kl_num : kl_num - *sr_inx;
    compressed_edgemap_hdr h;
    memset(&h, 0, sizeof h);
    h.edgemap_id = edgemap_id;
    h.nav = nav;
    h.kl_total = (uint32_t)kl_num;
    h.kl_num = (uint32_t)to_send;
    h.kl_id = (uint32_t)*sr_inx;
    h.paket_size = (uint16_t)(to_send * sizeof(compressed_kl) + sizeof(compressed_edgemap_hdr));
    h.rho_scale = rho_scale;
    const uint8_t *data = (const uint8_t *)(kls + *sr_inx);
    h.crc_em = crc16(data, (uint16_t)(to_send * sizeof(compressed_kl)));
    h.crc = crc16((const uint8_t *)&h, (uint16_t)(sizeof h - sizeof h.crc));
    pkt->resize(sizeof h + (size_t)to_send * sizeof(compressed_kl));
    memcpy(pkt->data(), &h, sizeof h);
    if (to_send) memcpy(pkt->data() + sizeof h, data, (size_t)to_send * sizeof(compressed_kl));
    *sr_inx += to_send;
    return to_send;
}

// ---- the receiving side ---------------------------------------------------------------------------------------------------------------
struct EdgeMap {     // what edgemap_com keeps of an edge map: records, id, scale, the pose it was taken at
    std::vector<compressed_kl> kls;
    int kl_num = 0;
    uint16_t edge_map_id = 0;
    float rho_scale = 1;
    em_compressed_nav_pkg em_pos = {};
};

struct Receiver {
    EdgeMap em;
    int keyline_max;
    explicit Receiver(int keyline_max_) : keyline_max(keyline_max_) {
        em.kls.assign((size_t)keyline_max, compressed_kl{0, 0, 0, 0});
        em.em_pos.K = 1;
    }
    // pkt[brecv]: the header followed by the records, as prepare_pkg lays them out.  false: the packet is discarded (size or header
    // CRC); true: accepted — *ready says a new edge map began and *copy_to (or null) got the finished one; records with a wrong data
    // CRC or an index past kl_total are left out, as the reference leaves them out.
    bool check_recv_pak(const uint8_t *pkt, int brecv, bool *ready, EdgeMap *copy_to = nullptr) {
        *ready = false;
        if (brecv < (int)sizeof(compressed_edgemap_hdr)) return false;   // (the reference reads the header from a buffer of its own)
        compressed_edgemap_hdr h;
        memcpy(&h, pkt, sizeof h);
        if (brecv != (int)h.paket_size || h.kl_total > (uint32_t)keyline_max) return false;
        if (h.crc != crc16((const uint8_t *)&h, (uint16_t)(sizeof h - sizeof h.crc))) return false;
        if (h.edgemap_id > em.edge_map_id) {
            if (copy_to) *copy_to = em;
            *ready = true;
            for (auto &k : em.kls) k.rho = 0;
            em.edge_map_id = h.edgemap_id;
            em.kl_num = (int)h.kl_total;
            em.em_pos = h.nav;
            em.rho_scale = h.rho_scale;
        } else if ((int)h.edgemap_id < (int)em.edge_map_id - 1) {
            em.edge_map_id = h.edgemap_id;
            em.kl_num = (int)h.kl_total;
        }
        const size_t bytes = (size_t)h.kl_num * sizeof(compressed_kl);
        if ((uint64_t)h.kl_id + h.kl_num <= h.kl_total && sizeof h + bytes <= (size_t)brecv &&
            h.crc_em == crc16(pkt + sizeof h, (uint16_t)bytes))
            memcpy(&em.kls[h.kl_id], pkt + sizeof h, bytes);
        return true;
    }
};

// getPair: the next segment from *pair_inx on, x_scaling / y_scaling as the sender's (0.5 and 1 in the reference)
inline bool get_pair(const compressed_kl *kls, int kl_num, float rho_scale, int *pair_inx, uncompressed_kl *kl0, uncompressed_kl *kl1,
                     double x_scaling = 0.5, double y_scaling = 1.0) {
    int &i = *pair_inx;
    const float rs = (float)(32767.0 / 20), ss = (float)(255.0 / 20);
    auto conv = [&](const compressed_kl &c, float rho, uncompressed_kl *o) {
        o->rho = rho;
        o->rho /= rs / rho_scale;
        o->x = (float)(c.x / x_scaling);
        o->y = (float)(c.y / y_scaling);
        o->s_rho = c.s_rho > 0 ? c.s_rho / ss : (float)1e-3;
    };
    for (; i < kl_num - 1 && kls[i].rho == 0; i++) {}
    if (i >= kl_num - 1) return false;
    conv(kls[i], (float)abs((int)kls[i].rho), kl0);
    i++;
    if (kls[i].rho == 0 || kls[i - 1].rho < 0) { *kl1 = *kl0; return true; }
    conv(kls[i], (float)kls[i].rho, kl1);
    if (kl1->rho < 0) { kl1->rho = -kl1->rho; i++; }
    return true;
}
inline int decode(const compressed_kl *kls, int kl_num, float rho_scale, std::vector<uncompressed_segment> *segs, int seg_max,
                  double x_scaling = 0.5, double y_scaling = 1.0) {
    segs->clear();
    int inx = 0;
    uncompressed_segment s;
    while ((int)segs->size() < seg_max && get_pair(kls, kl_num, rho_scale, &inx, &s.k0, &s.k1, x_scaling, y_scaling)) {
        s.visi_mask = true;
        segs->push_back(s);
    }
    return (int)segs->size();
}

}  // namespace edgemap
}  // namespace rebvo
