// net_keypoint.h — the wire format of an edge map for the reference's visualizer (include/CommLib/net_keypoint.h:38-78)
// and the packer that fills it (src/CommLib/net_keypoint.cpp:29-108).  Packing only: the UDP / TCP transport
// (src/CommLib/udp_port.cpp, edgemap_com.cpp) is device I/O this repository does not rebuild.
#ifndef REBVO_AMD_HOST_NET_KEYPOINT_H
#define REBVO_AMD_HOST_NET_KEYPOINT_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "rebvo/rebvo.h"

namespace rebvo {

constexpr double NET_RHO_SCALING = 10000.0;
constexpr double NET_POS_SCALING = 64.0;

#pragma pack(push, 1)
struct net_keyline {   // 15 bytes
    uint16_t qx, qy;       // rounded image position
    uint16_t rho, s_rho;   // inverse depth and its deviation, scaled by NET_RHO_SCALING / k_prof, at least 1
    int32_t n_kl;          // net index of the next KeyLine on the edge (-1: none)
    uint8_t m_num;
    union {
        struct { uint8_t x, y; } flow;               // matched displacement * 10 + 127 (or stereo disparity + 127)
        struct { unsigned a : 10; unsigned m : 6; } gradient;
    } extra;
};
#pragma pack(pop)
static_assert(sizeof(net_keyline) == 15, "net_keyline wire layout");

#pragma pack(push, 1)
struct compressed_nav_pkg {   // include/mtracklib/nav_data_defs.h: five float triples, two floats
    float Pos[3], Pose[3], Rot[3], Vel[3], G[3];
    float K, dt;
};
struct net_packet_hdr {       // include/CommLib/net_keypoint.h:64-78: what precedes the records and the picture in one packet
    int32_t data_size;        // header + kline_num records + jpeg_size
    int32_t w, h;
    int32_t key_num;
    int32_t jpeg_size;
    int32_t encoder_type;
    int32_t kline_num, km_num;
    float k, max_rho;
    compressed_nav_pkg nav;
};
#pragma pack(pop)
static_assert(sizeof(net_packet_hdr) == 108, "net_packet_hdr wire layout");

// hdr + hdr.kline_num records + hdr.jpeg_size bytes of picture, laid out as rebvo_third_t.cpp:219-234 sends them; data_size is set here.
// Returns the packet's length; `out` needs that much room (sizeof(net_packet_hdr) + 15 * kline_num + jpeg_size).
size_t build_net_packet(net_packet_hdr hdr, const net_keyline *records, const void *jpeg, unsigned char *out);

// The third thread's ring of EdgeMapDelay + 1 packets (rebvo_third_t.cpp:75-83, 189-246): the records of frame n (with their kline_num,
// km_num, k, max_rho) travel with the picture, size, encoder type and nav data of frame n + delay; the first `delay` packets carry no
// records.  push() takes one frame — hdr's record fields describe `records`, its other fields the picture — and returns that frame's packet.
class NetPacketRing {
public:
    explicit NetPacketRing(unsigned delay) : held(delay + 1) {}
    const std::vector<unsigned char> &push(const net_packet_hdr &hdr, const net_keyline *records, const void *jpeg);
private:
    struct Held { net_packet_hdr rec{}; std::vector<net_keyline> kl; };
    std::vector<Held> held;   // [frame % (delay + 1)]: records waiting for their picture
    size_t at = 0;
    std::vector<unsigned char> packet;
};

// Pack up to kl_size KeyLines of `from` (and, with a stereo pair map, the disparity of the stereo matches); sets every
// packed KeyLine's net_id.  Returns the number packed.
int copy_net_keyline(KeyLine *from, int kn, const KeyLine *from_pair, net_keyline *to, int kl_size, double k_prof);
// Second pass: n_kl = net index of each KeyLine's edge successor.
int copy_net_keyline_nextid(const KeyLine *from, int kn, net_keyline *to, int kl_size);

inline int copy_net_keyline(edge_tracker &from, edge_tracker *from_pair, net_keyline *to, int kl_size, double k_prof) {
    return copy_net_keyline(from.begin(), from.KNum(), from_pair ? from_pair->begin() : nullptr, to, kl_size, k_prof);
}
inline int copy_net_keyline_nextid(edge_tracker &from, net_keyline *to, int kl_size) {
    return copy_net_keyline_nextid(from.begin(), from.KNum(), to, kl_size);
}

}  // namespace rebvo

extern "C" {
/* flat view for non-C++ callers (tests): KeyLine arrays in the reference's 168-byte layout, 15-byte records out */
int rebvo_copy_net_keyline(void *keylines, int kn, const void *keylines_pair, void *out, int kl_size, double k_prof);
int rebvo_copy_net_keyline_nextid(const void *keylines, int kn, void *out, int kl_size);
/* hdr: a 108-byte net_packet_hdr whose kline_num and jpeg_size say how much of records / jpeg follows; returns the packet's length */
long long rebvo_build_net_packet(const void *hdr, const void *records, const void *jpeg, unsigned char *out);
/* rebvo::NetPacketRing: new(EdgeMapDelay), push one frame (-> the packet's length, written to out when it fits in cap), free */
void *rebvo_net_packet_ring_new(unsigned delay);
long long rebvo_net_packet_ring_push(void *ring, const void *hdr, const void *records, const void *jpeg, unsigned char *out, long long cap);
void rebvo_net_packet_ring_free(void *ring);
}
#endif
