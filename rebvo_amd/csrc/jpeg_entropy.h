// jpeg_entropy.h — the chain walk of the device JPEG decoder: Huffman stream -> quantised coefficients, written once for the device
// (k_jpeg_entropy, jpeg_decode.hip: every lane of a wave runs it on the same values) and for the CPU (the host decoder of
// rebvo_amd/host/src/jpeg_decode.cpp, tools/jpeg_entropy_guard.cpp).
//
// The only sequential chain in a JPEG is one restart interval.  A walk takes a run of whole intervals of one stream (a "group": the whole
// scan when the stream has no DRI), starts with zero DC predictions, and between two intervals of its run expects the RSTn marker whose
// number the interval's index gives.  It is bounded by construction:
//   - a byte is read only at a position below `len`, through Src::byte(pos);
//   - a block is handed to Sink::end_block(block) once per block of the group's MCUs, with block < Stream::nblocks, whatever the bits say;
//   - the outer loops run over the group's MCUs and their blocks, the AC loop at most 63 times, a code lookup at most 8 times, a refill at
//     most 4 times, and the fill bytes in front of a marker end at `len`.
// Status: 0, or the first failure — 1 an invalid code (or data where RSTn should stand), 2 out of data (the segment's end, or a marker
// that is not the expected RSTn, where bits are still needed), 3 a DC prediction or a dequantised coefficient outside what
// jpeg_reader.cpp accepts (|DC| < 2^15, |coefficient x quantiser| <= 2^24), 4 a run past the block's end (k > 63).  After a failure the
// walk decodes nothing more; the remaining blocks of the group still go to the sink, as zeros.
#pragma once
#include "rebvo/jpeg_decode.h"

namespace rebvo {
namespace jpegdec {

enum { kStInvalidCode = 1, kStOutOfData = 2, kStRange = 3, kStOverrun = 4 };
// what the walk tells Sink::note(what, value) about the stream's populations (the fixture generator counts them; the device sink ignores them)
enum { kNoteCodeLength = 0, kNoteDcCategory = 1, kNoteAcCategory = 2, kNoteZrl = 3, kNoteNoEob = 4 };
constexpr int kMaxGroups = 256;     // walks per stream at the most
constexpr int kMinGroupMcus = 32;   // a walk is worth a wave from about here on

// which restart intervals one walk takes, and where in the entropy-coded segment each walk starts
struct ChainPlan {
    int32_t ngroups, group_mcus;   // walk g takes the MCUs [g * group_mcus, min((g + 1) * group_mcus, mcux * mcuy))
    uint32_t off[kMaxGroups];      // its first byte, relative to the segment (the segment's length when the stream has too few markers)
};

// host: the RSTn markers of the segment give every group its start (one pass over the bytes)
inline void plan_chains(const uint8_t *ecs, const Stream &s, ChainPlan &p) {
    const int nmcu = s.mcux * s.mcuy;
    memset(&p, 0, sizeof p);
    if (s.restart <= 0 || s.restart >= nmcu) { p.ngroups = 1; p.group_mcus = nmcu; return; }
    const int nint = (nmcu + s.restart - 1) / s.restart;
    int per = (nint + kMaxGroups - 1) / kMaxGroups;                                            // intervals per group
    if (per * s.restart < kMinGroupMcus) per = (kMinGroupMcus + s.restart - 1) / s.restart;
    p.group_mcus = per * s.restart;
    p.ngroups = (nint + per - 1) / per;
    for (int g = 1; g < p.ngroups; g++) p.off[g] = s.ecs_len;
    int interval = 0;
    for (size_t e = 0; e + 1 < s.ecs_len;) {
        const uint8_t *f = (const uint8_t *)memchr(ecs + e, 0xFF, s.ecs_len - 1 - e);
        if (!f) break;
        e = (size_t)(f - ecs);
        const unsigned x = ecs[e + 1];
        if (x >= 0xD0 && x <= 0xD7) {
            interval++;
            if (interval % per == 0 && interval / per < p.ngroups) p.off[interval / per] = (uint32_t)(e + 2);
            e += 2;
        } else e += (x == 0xFF) ? 1 : 2;
    }
}

struct BitReader {
    uint32_t acc;   // the low n bits are the stream's next bits
    int n;
    uint32_t pos, len;
    bool ended;     // the data ends at pos: the segment's end or a marker (left in place)
};

template <class Src>
REBVO_JD_HD inline void br_fill(BitReader &b, Src &src) {
    for (int i = 0; i < 4 && b.n <= 24 && !b.ended; i++) {
        if (b.pos >= b.len) { b.ended = true; break; }
        const uint32_t c = (uint32_t)src.byte(b.pos);
        if (c == 0xFF) {
            if (b.pos + 1 < b.len && src.byte(b.pos + 1) == 0) b.pos += 2;   // a stuffed byte
            else { b.ended = true; break; }
        } else b.pos++;
        b.acc = (b.acc << 8) | c;
        b.n += 8;
    }
}

// the next symbol of table t (its code's length to `l`), or -status
template <class Src>
REBVO_JD_HD inline int br_symbol(BitReader &b, Src &src, const Huff &t, int &l) {
    br_fill(b, src);
    const uint32_t peek = b.n >= 16 ? (b.acc >> (b.n - 16)) & 0xFFFFu : (b.acc << (16 - b.n)) & 0xFFFFu;   // the bits behind the data are zeros
    int sym = 0;
    l = 0;
    const uint32_t e = t.look[peek >> 8];
    if (e) { l = (int)(e >> 8); sym = (int)(e & 0xFF); }
    else {
        for (int k = 9; k <= 16; k++) {
            const int code = (int)(peek >> (16 - k));
            if (code <= t.maxcode[k]) {
                const int at = t.valoff[k] + code;
                if (at < 0 || at > 255) return -kStInvalidCode;
                l = k; sym = t.vals[at];
                break;
            }
        }
        if (!l) return -kStInvalidCode;
    }
    if (l > b.n) return -kStOutOfData;
    b.n -= l;
    return sym;
}

// s bits (1 .. 15) as a signed value of category s (T.81 F.2.2.1: EXTEND), or out of data
template <class Src>
REBVO_JD_HD inline int br_receive_extend(BitReader &b, Src &src, int s, int &v) {
    if (b.n < s) br_fill(b, src);
    if (b.n < s) return kStOutOfData;
    b.n -= s;
    const int u = (int)((b.acc >> b.n) & ((1u << s) - 1u));
    v = u < (1 << (s - 1)) ? u - (1 << s) + 1 : u;
    return 0;
}

REBVO_JD_HD inline bool dequant_in_range(int v, int q) {
    const long long x = (long long)v * q;
    return x >= -(1 << 24) && x <= (1 << 24);
}

template <class Src, class Sink>
REBVO_JD_HD inline int decode_block(BitReader &b, Src &src, const Huff &dc, const Huff &ac, const uint16_t *q, int &pred, Sink &sink) {
    int l = 0;
    const int t = br_symbol(b, src, dc, l);
    if (t < 0) return -t;
    if (t > 11) return kStInvalidCode;
    sink.note(kNoteCodeLength, l);
    sink.note(kNoteDcCategory, t);
    if (t) {
        int diff = 0;
        if (int e = br_receive_extend(b, src, t, diff)) return e;
        pred += diff;
    }
    if (pred < -32768 || pred > 32767 || !dequant_in_range(pred, q[0])) return kStRange;
    sink.put(0, pred);
    int k = 1;
    for (int it = 0; it < 63 && k < 64; it++) {
        const int rs = br_symbol(b, src, ac, l);
        if (rs < 0) return -rs;
        sink.note(kNoteCodeLength, l);
        const int r = rs >> 4, sz = rs & 15;
        if (sz == 0) {
            if (r != 15) return 0;   // EOB
            sink.note(kNoteZrl, 1);
            k += 16;
            continue;
        }
        k += r;
        if (k > 63) return kStOverrun;
        int v = 0;
        if (int e = br_receive_extend(b, src, sz, v)) return e;
        const int nat = zigzag(k);
        if (!dequant_in_range(v, q[nat])) return kStRange;
        sink.note(kNoteAcCategory, sz);
        sink.put(nat, v);
        k++;
    }
    sink.note(kNoteNoEob, 1);
    return 0;
}

// between two intervals of a group: the padding bits go, RST<n> must follow (fill bytes in front of it are allowed)
template <class Src>
REBVO_JD_HD inline int next_interval(BitReader &b, Src &src, int n) {
    if (b.n >= 8) return kStInvalidCode;   // whole bytes of data are left over
    b.acc = 0; b.n = 0; b.ended = false;
    if (b.pos >= b.len) return kStOutOfData;
    if (src.byte(b.pos) != 0xFF) return kStInvalidCode;
    uint32_t p = b.pos + 1;
    while (p < b.len && src.byte(p) == 0xFF) p++;
    if (p >= b.len || src.byte(p) != 0xD0 + n) return kStOutOfData;
    b.pos = p + 1;
    return 0;
}

// One group of stream s: its MCUs [mcu_first, mcu_first + mcu_count), mcu_first a multiple of the restart interval, from byte `pos` of the
// segment's `len` bytes.  Src: int byte(uint32_t pos).  Sink: begin_block(), put(natural index, value), note(what, value), end_block(block).  *end_pos: the
// first byte the walk has not consumed.
template <class Src, class Sink>
REBVO_JD_HD inline int chain_walk(const Stream &s, int mcu_first, int mcu_count, uint32_t pos, uint32_t len, Src &src, Sink &sink, uint32_t *end_pos) {
    BitReader b = {0u, 0, pos, len, false};
    int pred[3] = {0, 0, 0}, status = 0;
    int until = s.restart > 0 ? s.restart : mcu_count;
    int interval = s.restart > 0 ? mcu_first / s.restart : 0;
    for (int m = 0; m < mcu_count; m++) {
        if (until == 0) {
            if (!status) status = next_interval(b, src, interval & 7);
            interval++;
            pred[0] = pred[1] = pred[2] = 0;
            until = s.restart;
        }
        until--;
        const int mcu = mcu_first + m, my = mcu / s.mcux, mx = mcu - my * s.mcux;
        for (int ci = 0; ci < s.ncomp; ci++) {
            const Comp &c = s.comp[ci];
            for (int by = 0; by < c.v; by++)
                for (int bx = 0; bx < c.h; bx++) {
                    sink.begin_block();
                    if (!status) status = decode_block(b, src, s.dc[c.td], s.ac[c.ta], s.q[c.tq], pred[ci], sink);
                    sink.end_block(c.block_base + (my * c.v + by) * c.wblocks + mx * c.h + bx);
                }
        }
    }
    if (end_pos) *end_pos = b.pos;
    return status;
}

}  // namespace jpegdec
}  // namespace rebvo
