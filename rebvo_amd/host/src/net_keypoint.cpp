// net_keypoint.cpp — see rebvo/net_keypoint.h (reference: src/CommLib/net_keypoint.cpp:29-108).
#include "rebvo/net_keypoint.h"

#include <algorithm>
#include <cmath>

namespace rebvo {

namespace {
// util::clamp_uchar / clamp_ushort (include/UtilLib/util.h:52-66): the argument arrives as float
inline uint8_t clamp_uchar(float f) { return f < 0 ? 0 : f > 255.0 ? 255 : (uint8_t)f; }
inline uint16_t clamp_ushort(float f) {
    if (f < 0) return 0;
    if (f > 65535.0) return 65535;
    return (uint16_t)f;
}
}  // namespace

int copy_net_keyline(KeyLine *from, int kn, const KeyLine *from_pair, net_keyline *to, int kl_size, double k_prof) {
    int j = 0;
    for (int i = 0; i < kn; i++) {
        KeyLine &kl = from[i];
        if (j >= kl_size) break;
        to[j].qx = (uint16_t)std::round(kl.c_p.x);
        to[j].qy = (uint16_t)std::round(kl.c_p.y);
        to[j].rho = std::max(clamp_ushort((float)(NET_RHO_SCALING * kl.rho / k_prof)), (uint16_t)1);
        to[j].s_rho = std::max(clamp_ushort((float)(NET_RHO_SCALING * kl.s_rho / k_prof)), (uint16_t)1);
        if (from_pair) {
            if (kl.stereo_m_id >= 0 && std::fabs(std::round(-kl.c_p.x + from_pair[kl.stereo_m_id].c_p.x)) < 127 &&
                std::fabs(std::round(-kl.c_p.y + from_pair[kl.stereo_m_id].c_p.y)) < 127) {
                to[j].extra.flow.x = clamp_uchar((float)std::round((-kl.c_p.x + from_pair[kl.stereo_m_id].c_p.x) + 127.0));
                to[j].extra.flow.y = clamp_uchar((float)std::round((-kl.c_p.y + from_pair[kl.stereo_m_id].c_p.y) + 127.0));
            } else {
                to[j].extra.flow.x = 127;
                to[j].extra.flow.y = 127;
            }
        } else {
            to[j].extra.flow.x = clamp_uchar((float)std::round((kl.p_m.x - kl.p_m_0.x) * 10 + 127.0));
            to[j].extra.flow.y = clamp_uchar((float)std::round((kl.p_m.y - kl.p_m_0.y) * 10 + 127.0));
        }
        to[j].n_kl = -1;
        to[j].m_num = clamp_uchar((float)kl.m_num);
        kl.net_id = j;
        j++;
    }
    return j;
}

int copy_net_keyline_nextid(const KeyLine *from, int kn, net_keyline *to, int kl_size) {
    int j = 0;
    for (int i = 0; i < kn; i++) {
        const KeyLine &kl = from[i];
        if (j >= kl_size) break;   // as in the reference: tested against the PREVIOUS KeyLine's net index
        j = kl.net_id;
        if (j < 0 || j >= kl_size) continue;   // not packed (the reference would index out of bounds here)
        if (kl.n_id >= 0) to[j].n_kl = from[kl.n_id].net_id;
    }
    return j;
}

size_t build_net_packet(net_packet_hdr hdr, const net_keyline *records, const void *jpeg, unsigned char *out) {
    const size_t nrec = hdr.kline_num > 0 ? (size_t)hdr.kline_num : 0, njpg = hdr.jpeg_size > 0 ? (size_t)hdr.jpeg_size : 0;
    const size_t hdr_payload = sizeof(net_packet_hdr) + sizeof(net_keyline) * nrec;
    hdr.kline_num = (int32_t)nrec;
    hdr.jpeg_size = (int32_t)njpg;
    hdr.data_size = (int32_t)(hdr_payload + njpg);
    std::memcpy(out, &hdr, sizeof hdr);
    if (nrec) std::memcpy(out + sizeof hdr, records, sizeof(net_keyline) * nrec);
    if (njpg) std::memcpy(out + hdr_payload, jpeg, njpg);
    return hdr_payload + njpg;
}

const std::vector<unsigned char> &NetPacketRing::push(const net_packet_hdr &hdr, const net_keyline *records, const void *jpeg) {
    // this frame's records wait in the entry BEFORE the current one (it comes up again `delay` frames from now) ...
    Held &rec = held[(at + held.size() - 1) % held.size()];
    rec.rec = hdr;
    rec.kl.assign(records, records + (hdr.kline_num > 0 ? hdr.kline_num : 0));
    // ... and the current entry's records, written `delay` frames ago (none yet: a zeroed header), leave with this frame's picture
    const Held &cur = held[at];
    net_packet_hdr h = hdr;
    h.key_num = cur.rec.key_num;
    h.kline_num = (int32_t)cur.kl.size();
    h.km_num = cur.rec.km_num;
    h.k = cur.rec.k;
    h.max_rho = cur.rec.max_rho;
    packet.resize(sizeof(net_packet_hdr) + sizeof(net_keyline) * cur.kl.size() + (hdr.jpeg_size > 0 ? hdr.jpeg_size : 0));
    build_net_packet(h, cur.kl.data(), jpeg, packet.data());
    at = (at + 1) % held.size();
    return packet;
}

}  // namespace rebvo

extern "C" {
long long rebvo_build_net_packet(const void *hdr, const void *records, const void *jpeg, unsigned char *out) {
    rebvo::net_packet_hdr h;
    std::memcpy(&h, hdr, sizeof h);
    return (long long)rebvo::build_net_packet(h, (const rebvo::net_keyline *)records, jpeg, out);
}
void *rebvo_net_packet_ring_new(unsigned delay) { return new rebvo::NetPacketRing(delay); }
long long rebvo_net_packet_ring_push(void *ring, const void *hdr, const void *records, const void *jpeg, unsigned char *out, long long cap) {
    rebvo::net_packet_hdr h;
    std::memcpy(&h, hdr, sizeof h);
    const std::vector<unsigned char> &p = ((rebvo::NetPacketRing *)ring)->push(h, (const rebvo::net_keyline *)records, jpeg);
    if (out && (long long)p.size() <= cap) std::memcpy(out, p.data(), p.size());
    return (long long)p.size();
}
void rebvo_net_packet_ring_free(void *ring) { delete (rebvo::NetPacketRing *)ring; }
int rebvo_copy_net_keyline(void *keylines, int kn, const void *keylines_pair, void *out, int kl_size, double k_prof) {
    return rebvo::copy_net_keyline((rebvo::KeyLine *)keylines, kn, (const rebvo::KeyLine *)keylines_pair, (rebvo::net_keyline *)out, kl_size, k_prof);
}
int rebvo_copy_net_keyline_nextid(const void *keylines, int kn, void *out, int kl_size) {
    return rebvo::copy_net_keyline_nextid((const rebvo::KeyLine *)keylines, kn, (rebvo::net_keyline *)out, kl_size);
}
}
