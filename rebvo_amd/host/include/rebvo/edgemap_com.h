// edgemap_com.h — the reference's compressed edge map on the host (include/CommLib/edgemap_com.h, src/CommLib/edgemap_com.cpp), header-only:
//   rebvo_compress_edgemap   edgemap_com_sender::compress_edgemap (:168-326) as the straight serial loop over an AoS KeyLine list, on
//                            the walk and the fit the device runs (csrc/edgemap_fit.h); what edgehip_edgemap_compress is tested against
//   compressed_kl, em_compressed_nav_pkg, compressed_edgemap_hdr   the wire structs (edgemap_com.h:45-102), packed
//   crc16                    util::CRC16 (src/UtilLib/libcrc.cpp): the reflected 0xA001 polynomial from 0xFFFF, table generated here
//   prepare_pkg              edgemap_com_sender::PreparePkg (:329-353): header with both CRC-16 fields + the records of one packet
//   Receiver::check_recv_pak edgemap_com_receiver::CheckRecvPak (:374-429)
//   get_pair / decode        edgemap_com::getPair (:46-86), edgemap_com_decoder::Decode (:431-440)
//   update_pos               edgemap_com::UpdatePos (:142-160): DPose, DPos, DK of a stored map seen from a new view (the trigonometry of
//                            the receiving side; the device takes its result)
//   transform_pos / hide_visible   edgemap_com::TransformPos (:106-127), edgemap_com_decoder::HideVisible (:443-473)
//   fill_depth_map           edgemap_com_decoder::fillDepthMap (:475-528) onto a plain grid, serially; what edgehip_depth_fill_segments is
//                            tested against.  The per-segment and per-step rules are csrc/edgemap_seg.h, which the device runs too.
#pragma once
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <stdlib.h>
#include <vector>

#include "edgehip.h"
#include "edgemap_fit.h"
#include "edgemap_seg.h"
#include "linalg.h"

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

// Decode through the local rule of edgemap_seg.h (what k_em_decode runs): equal to decode() on every list
inline int decode_local(const compressed_kl *kls, int kl_num, float rho_scale, std::vector<uncompressed_segment> *segs, int seg_max,
                        double x_scaling = 0.5, double y_scaling = 1.0) {
    segs->clear();
    for (int i = 0; i < kl_num && (int)segs->size() < seg_max; i++) {
        if (!seg_starts(i >= 1 ? kls[i - 1].rho : 0, kls[i].rho, i, kl_num)) continue;
        SegPoint k0, k1;
        seg_pair(kls[i].x, kls[i].y, kls[i].rho, kls[i].s_rho, kls[i + 1].x, kls[i + 1].y, kls[i + 1].rho, kls[i + 1].s_rho, rho_scale, x_scaling,
                 y_scaling, &k0, &k1);
        uncompressed_segment s;
        s.k0 = {k0.x, k0.y, k0.rho, k0.s_rho};
        s.k1 = {k1.x, k1.y, k1.rho, k1.s_rho};
        s.visi_mask = true;
        segs->push_back(s);
    }
    return (int)segs->size();
}

// ---- UpdatePos: the stored map (em_pos) seen from a new view (new_pos) ------------------------------------------------------------------
struct PosDelta {
    double DPose[9];   // Rn^T Ro, row-major
    double DPos[3];    // Rn^T (Vo - Vn)
    double DK;         // em_pos.K
};
// TooN::SO3<>::exp on the Vector<3, float> that makeVector(w[0], w[1], w[2]) makes of a nav package's floats (so3.h:203-285): theta_sq
// and the mixed products w[i] * w[j] are float there, everything else double.  For float input this is what la::so3_exp restates for
// double input; the branch structure is the same.
inline la::Mat<3, 3> so3_exp_float(const float w[3]) {
    const double one_6th = 1.0 / 6.0, one_20th = 1.0 / 20.0;
    float dotf = 0;
    for (int i = 0; i < 3; i++) dotf += w[i] * w[i];
    const double theta_sq = dotf, theta = sqrt(theta_sq);
    double A, B;
    if (theta_sq < 1e-8) {
        A = 1.0 - one_6th * theta_sq;
        B = 0.5;
    } else if (theta_sq < 1e-6) {
        B = 0.5 - 0.25 * one_6th * theta_sq;
        A = 1.0 - theta_sq * one_6th * (1.0 - one_20th * theta_sq);
    } else {
        const double inv_theta = 1.0 / theta;
        A = sin(theta) * inv_theta;
        B = (1 - cos(theta)) * (inv_theta * inv_theta);
    }
    la::Mat<3, 3> R;
    const double wx2 = (double)w[0] * w[0], wy2 = (double)w[1] * w[1], wz2 = (double)w[2] * w[2];
    R(0, 0) = 1.0 - B * (wy2 + wz2);
    R(1, 1) = 1.0 - B * (wx2 + wz2);
    R(2, 2) = 1.0 - B * (wx2 + wy2);
    double a = A * w[2], b = B * (w[0] * w[1]);
    R(0, 1) = b - a; R(1, 0) = b + a;
    a = A * w[1]; b = B * (w[0] * w[2]);
    R(0, 2) = b + a; R(2, 0) = b - a;
    a = A * w[0]; b = B * (w[1] * w[2]);
    R(1, 2) = b - a; R(2, 1) = b + a;
    return R;
}
inline PosDelta update_pos(const em_compressed_nav_pkg &em_pos, const em_compressed_nav_pkg &new_pos) {
    const la::Mat<3, 3> Rn = so3_exp_float(new_pos.w), Ro = so3_exp_float(em_pos.w);
    const la::Mat<3, 3> RnT = la::transpose(Rn);
    PosDelta d;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) {
            double s = 0;
            for (int k = 0; k < 3; k++) s += RnT(r, k) * Ro(k, c);
            d.DPose[3 * r + c] = s;
        }
        double s = 0;
        for (int k = 0; k < 3; k++) s += RnT(r, k) * ((double)em_pos.p[k] - (double)new_pos.p[k]);
        d.DPos[r] = s;
    }
    d.DK = em_pos.K;
    return d;
}

struct Camera {        // what the decoder reads of cam_model: pp (float), zfm (double), sz
    float ppx, ppy;
    double zfm;
    int w, h;
    SegCam seg() const { SegCam c; c.ppx = ppx; c.ppy = ppy; c.zfm = zfm; c.w = (uint32_t)w; c.h = (uint32_t)h; return c; }
};
inline SegPoint as_point(const uncompressed_kl &k) { return SegPoint{k.x, k.y, k.rho, k.s_rho}; }

inline uncompressed_kl transform_pos(const uncompressed_kl &p, const PosDelta &d, float k_em, float k_new, const Camera &cam) {
    const SegPoint t = seg_transform_pos(as_point(p), d.DPose, d.DPos, k_em, k_new, cam.seg());
    return uncompressed_kl{t.x, t.y, t.rho, t.s_rho};
}
// HideVisible with UpdatePos(pos) already applied (d): clears the flag of every visible segment the new view sees; a cleared flag
// stays cleared.  Returns s_num: the segments that were visible and stay visible.
inline int hide_visible(uncompressed_segment *segs, int seg_num, const PosDelta &d, float k_em, float k_new, const Camera &cam) {
    int s_num = 0;
    const SegCam c = cam.seg();
    for (int i = 0; i < seg_num; i++) {
        if (!segs[i].visi_mask) continue;
        if (seg_seen(as_point(segs[i].k0), as_point(segs[i].k1), d.DPose, d.DPos, k_em, k_new, c)) segs[i].visi_mask = false;
        else s_num++;
    }
    return s_num;
}

// ---- fillDepthMap onto a plain grid -----------------------------------------------------------------------------------------------------
struct DepthGrid {     // depth_filler's cells: size = image size / block size, cell (x, y) at y * gw + x
    int gw, gh, bw, bh;
    std::vector<double> rho, s_rho, I_rho;
    std::vector<uint8_t> fixed;
    DepthGrid(int w, int h, int bw_, int bh_) : gw(w / bw_), gh(h / bh_), bw(bw_), bh(bh_) { reset(); }
    void reset() {     // depth_filler::ResetData (depth_filler.cpp:41-56)
        const size_t G = (size_t)(gw > 0 ? gw : 0) * (size_t)(gh > 0 ? gh : 0);
        rho.assign(G, 1.0);
        s_rho.assign(G, 40.0);
        I_rho.assign(G, 1.0 / (40.0 * 40.0));
        fixed.assign(G, 0);
    }
};
// Every segment in list order, every step in step order, one update per step.  use_visibility: skip hidden segments (this library's
// extension; the reference reads the records again and knows no flags).  gates[seg_num] (or null): the SegGate of every segment.
// Returns the number of steps folded.
inline long long fill_depth_map(const uncompressed_segment *segs, int seg_num, DepthGrid *g, const Camera &cam, double v_thresh, double a_thresh_deg,
                                bool use_visibility = false, int *gates = nullptr) {
    const double cos_a = cos(a_thresh_deg * M_PI / 180.0);
    const SegCam c = cam.seg();
    long long steps = 0;
    for (int j = 0; j < seg_num; j++) {
        int gate = -1;
        if (!(use_visibility && !segs[j].visi_mask)) {
            const SegSteps s = seg_steps(as_point(segs[j].k0), as_point(segs[j].k1), c, v_thresh, cos_a, &gate);
            for (int i = 0; i < s.n; i++) {
                const size_t cell = (size_t)seg_step_cell(s, i, g->bw, g->bh, g->gw, g->gh);
                seg_fold(seg_step_rho(s, i), s.kl_I, &g->rho.at(cell), &g->s_rho.at(cell), &g->I_rho.at(cell));
                g->fixed.at(cell) = 1;
                steps++;
            }
        }
        if (gates) gates[j] = gate;
    }
    return steps;
}

}  // namespace edgemap
}  // namespace rebvo
