// jpeg_decode.h — the marker parser of the device JPEG decoder (rebvo_amd/csrc/jpeg_decode.hip), header-only and shared by the device
// library, the mirror library and the tools.  It reads one stream from SOI to its first SOS into a plain descriptor: the frame, its
// components, the quantisers in natural order, the Huffman tables in the form the chain walk (csrc/jpeg_entropy.h) looks codes up in, the
// restart interval, and where the entropy-coded segment lies.  A stream the device does not decode gets a reason code, never a crash:
// every read is checked against the stream's length.
//
// Decodable on the device: SOF0 / SOF1 (Huffman, 8-bit samples), one scan over every component, grey or YCbCr in 4:4:4, 4:2:2 (h2v1) or
// 4:2:0 (h2v2), any DHT tables, any restart interval.  The pixel rules are the host reader's (src/jpeg_reader.cpp), i.e. libjpeg's.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define REBVO_JD_HD __host__ __device__
#else
#define REBVO_JD_HD
#endif

namespace rebvo {
namespace jpegdec {

enum Reason {
    kOk = 0,
    kTruncated = 1,     // not a JPEG, or the stream ends before its scan header is complete
    kProgressive = 2,   // SOF2
    kCoding = 3,        // lossless, hierarchical or arithmetic-coded (SOF3, SOF5 .. SOF15)
    kPrecision = 4,     // not 8-bit samples
    kComponents = 5,    // neither 1 nor 3 components (CMYK)
    kSampling = 6,      // not grey / 4:4:4 / 4:2:2 (h2v1) / 4:2:0 (h2v2): 4:4:0 and everything rarer
    kMultiScan = 7,     // the first scan does not carry every component, or something other than EOI follows it
    kColourSpace = 8,   // three components that are not YCbCr (Adobe transform 0, or the ids 'R' 'G' 'B')
    kTable = 9,         // a table the scan names is missing, or a DHT that is no prefix code
    kHeader = 10,       // a malformed marker segment
    kSize = 11,         // (edgehip_upload_jpeg) not the context's w x h
    kTooLong = 12       // (edgehip_upload_jpeg) the entropy-coded segment is longer than cap_bytes
};

// A Huffman table as the walk reads it: the next 8 bits index `look` ((length << 8) | symbol, 0: the code is longer); a longer code is
// found by libjpeg's maxcode walk over lengths 9 .. 16 and read at vals[valoff[l] + code].
struct Huff {
    uint16_t look[256];
    int32_t maxcode[17];   // [l], l = 1 .. 16: the largest code of length l, -1 when there is none
    int32_t valoff[17];    // [l]: index of the first symbol of length l minus its code
    uint8_t vals[256];
    int32_t set;
};

struct Comp {
    int32_t id, h, v, tq, td, ta;
    int32_t wblocks, hblocks;   // blocks per row and block rows as coded (whole MCUs)
    int32_t cw, ch;             // the component's true size in samples: ceil(image * sampling / max sampling)
    int32_t block_base;         // first block of the component in the stream's coefficient and sample planes
    int32_t pad;
};

struct Stream {
    int32_t w, h, ncomp, restart, reason;
    uint32_t ecs_off, ecs_len;   // the entropy-coded segment: from behind the scan header up to the first marker that is not RSTn
    int32_t hmax, vmax, mcux, mcuy, nblocks;
    Comp comp[3];
    uint16_t q[4][64];           // natural order
    int32_t q_set[4];
    Huff dc[4], ac[4];
};
static_assert(sizeof(Stream) % 16 == 0, "copied in 16-byte words");

// what edgehip_jpeg_probe gives out (the same layout as edgehip_jpeg_info)
struct Info {
    int32_t w, h, components, hsamp, vsamp, restart_interval;
    uint32_t entropy_offset, entropy_length;
    int32_t reason;
};

REBVO_JD_HD inline int zigzag(int k) {   // position in the zig-zag sequence -> natural index
    constexpr uint8_t t[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return t[k & 63];
}

// counts[16], vals[total]: false when the lengths are no prefix code (more codes of a length than the code space has left)
inline bool build_huff(Huff &t, const uint8_t *counts, const uint8_t *vals, int total) {
    memset(&t, 0, sizeof t);
    if (total > 256) return false;
    int code = 0, k = 0;
    for (int l = 1; l <= 16; l++) {
        const int cnt = counts[l - 1];
        t.valoff[l] = k - code;
        t.maxcode[l] = cnt ? code + cnt - 1 : -1;
        if (code + cnt > (1 << l)) return false;
        if (l <= 8)
            for (int i = 0; i < cnt; i++)
                for (int f = 0; f < (1 << (8 - l)); f++) t.look[((code + i) << (8 - l)) + f] = (uint16_t)((l << 8) | vals[k + i]);
        code = (code + cnt) << 1;
        k += cnt;
    }
    if (k != total) return false;
    memcpy(t.vals, vals, (size_t)total);
    t.set = 1;
    return true;
}

// The stream's markers up to the first SOS -> s; s.reason says whether the device decodes it.  Returns s.reason.
inline int parse(const uint8_t *d, size_t len, Stream &s) {
    memset(&s, 0, sizeof s);
    auto fail = [&](int r) { s.reason = r; return r; };
    if (!d || len < 4 || d[0] != 0xFF || d[1] != 0xD8) return fail(kTruncated);
    size_t pos = 2;
    bool have_sof = false;
    int adobe = -1;
    for (;;) {
        if (pos + 2 > len) return fail(kTruncated);
        if (d[pos] != 0xFF) return fail(kHeader);
        while (pos < len && d[pos] == 0xFF) pos++;   // fill bytes
        if (pos >= len) return fail(kTruncated);
        const unsigned m = d[pos++];
        if (m == 0xD9) return fail(kTruncated);      // EOI before any scan
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7) || m == 0xD8) continue;
        if (pos + 2 > len) return fail(kTruncated);
        const size_t sl = (size_t)d[pos] << 8 | d[pos + 1];
        if (sl < 2) return fail(kHeader);
        if (pos + sl > len) return fail(kTruncated);
        const uint8_t *p = d + pos + 2;
        const size_t n = sl - 2;
        if (m == 0xDB) {   // DQT
            size_t o = 0;
            while (o < n) {
                const int pq = p[o] >> 4, tq = p[o] & 15;
                o++;
                if (tq > 3 || pq > 1 || o + (pq ? 128u : 64u) > n) return fail(kHeader);
                for (int i = 0; i < 64; i++) {
                    s.q[tq][zigzag(i)] = pq ? (uint16_t)(p[o] << 8 | p[o + 1]) : p[o];
                    o += pq ? 2 : 1;
                }
                s.q_set[tq] = 1;
            }
        } else if (m == 0xC4) {   // DHT
            size_t o = 0;
            while (o < n) {
                if (o + 17 > n) return fail(kHeader);
                const int tc = p[o] >> 4, th = p[o] & 15;
                int total = 0;
                for (int i = 0; i < 16; i++) total += p[o + 1 + i];
                if (tc > 1 || th > 3 || o + 17 + (size_t)total > n) return fail(kHeader);
                if (!build_huff(tc ? s.ac[th] : s.dc[th], p + o + 1, p + o + 17, total)) return fail(kTable);
                o += 17 + (size_t)total;
            }
        } else if (m == 0xC0 || m == 0xC1) {   // SOF0 / SOF1
            if (have_sof || n < 6) return fail(kHeader);
            if (p[0] != 8) return fail(kPrecision);
            s.h = p[1] << 8 | p[2];
            s.w = p[3] << 8 | p[4];
            s.ncomp = p[5];
            if (s.ncomp != 1 && s.ncomp != 3) return fail(kComponents);
            if (n < 6u + 3u * (unsigned)s.ncomp || s.w < 1 || s.h < 1 || s.w > 16384 || s.h > 16384) return fail(kHeader);
            for (int i = 0; i < s.ncomp; i++) {
                Comp &c = s.comp[i];
                c.id = p[6 + 3 * i]; c.h = p[7 + 3 * i] >> 4; c.v = p[7 + 3 * i] & 15; c.tq = p[8 + 3 * i];
                if (c.tq > 3 || c.h < 1 || c.v < 1) return fail(kHeader);
                if (c.h > 4 || c.v > 4) return fail(kHeader);
            }
            have_sof = true;
        } else if (m == 0xC2) {
            return fail(kProgressive);
        } else if (m >= 0xC3 && m <= 0xCF && m != 0xC8) {   // (C4 was taken above; CC, DAC, belongs to the arithmetic coder too)
            return fail(kCoding);
        } else if (m == 0xDD) {
            if (n < 2) return fail(kHeader);
            s.restart = p[0] << 8 | p[1];
        } else if (m == 0xEE) {
            if (n >= 12 && !memcmp(p, "Adobe", 5)) adobe = p[11];
        } else if (m == 0xDA) {   // SOS: the frame's geometry, the scan's tables, the entropy-coded segment
            if (!have_sof || n < 1) return fail(kHeader);
            const int ns = p[0];
            if (ns < 1 || ns > 4 || n < 1u + 2u * (unsigned)ns + 3u) return fail(kHeader);
            if (ns != s.ncomp) return fail(kMultiScan);
            for (int i = 0; i < ns; i++) {
                Comp &c = s.comp[i];
                if (p[1 + 2 * i] != c.id) return fail(kMultiScan);   // (a scan that orders its components differently)
                c.td = p[2 + 2 * i] >> 4; c.ta = p[2 + 2 * i] & 15;
                if (c.td > 3 || c.ta > 3) return fail(kHeader);
                if (!s.q_set[c.tq] || !s.dc[c.td].set || !s.ac[c.ta].set) return fail(kTable);
            }
            if (p[1 + 2 * ns] != 0 || p[2 + 2 * ns] != 63 || p[3 + 2 * ns] != 0) return fail(kHeader);
            if (s.ncomp == 1) {
                s.comp[0].h = s.comp[0].v = 1;   // one component alone: its blocks in raster order, whatever factors it names
            } else {
                const Comp &y = s.comp[0];
                const bool ok = s.comp[1].h == 1 && s.comp[1].v == 1 && s.comp[2].h == 1 && s.comp[2].v == 1 &&
                                ((y.h == 1 && y.v == 1) || (y.h == 2 && y.v == 1) || (y.h == 2 && y.v == 2));
                if (!ok) return fail(kSampling);
                if (adobe == 0 || (s.comp[0].id == 'R' && s.comp[1].id == 'G' && s.comp[2].id == 'B')) return fail(kColourSpace);
            }
            s.hmax = s.comp[0].h; s.vmax = s.comp[0].v;
            s.mcux = (s.w + 8 * s.hmax - 1) / (8 * s.hmax);
            s.mcuy = (s.h + 8 * s.vmax - 1) / (8 * s.vmax);
            s.nblocks = 0;
            for (int i = 0; i < s.ncomp; i++) {
                Comp &c = s.comp[i];
                c.wblocks = s.mcux * c.h; c.hblocks = s.mcuy * c.v;
                c.cw = (s.w * c.h + s.hmax - 1) / s.hmax; c.ch = (s.h * c.v + s.vmax - 1) / s.vmax;
                c.block_base = s.nblocks;
                s.nblocks += c.wblocks * c.hblocks;
            }
            size_t e = pos + sl;
            s.ecs_off = (uint32_t)e;
            while (e < len) {   // up to the first marker that is neither a stuffed FF 00, a fill byte nor RSTn
                const uint8_t *f = (const uint8_t *)memchr(d + e, 0xFF, len - e);
                if (!f) { e = len; break; }
                e = (size_t)(f - d);
                if (e + 1 >= len) { e = len; break; }   // a cut FF: the walk meets it as the end of its data
                const unsigned x = d[e + 1];
                if (x == 0x00 || (x >= 0xD0 && x <= 0xD7)) e += 2;
                else if (x == 0xFF) e += 1;
                else break;
            }
            s.ecs_len = (uint32_t)(e - s.ecs_off);
            // one scan, then EOI (or the end of a cut stream, which the walk reports): a further scan, tables or a DNL behind the data
            // belong to files the host reader takes
            if (e < len && d[e + 1] != 0xD9) return fail(kMultiScan);
            return s.reason = kOk;
        }
        pos += sl;
    }
}

// What every caller with a frame size of its own applies to a parsed descriptor: a stream that is not w x h gets kSize, one whose
// entropy-coded segment exceeds cap_bytes (0: no cap) kTooLong; an earlier reason stays.  Returns s.reason.
inline int expect(Stream &s, int w, int h, uint32_t cap_bytes) {
    if (!s.reason && (s.w != w || s.h != h)) s.reason = kSize;
    if (!s.reason && cap_bytes && s.ecs_len > cap_bytes) s.reason = kTooLong;
    return s.reason;
}

inline Info info_of(const Stream &s) {
    Info i;
    i.w = s.w; i.h = s.h; i.components = s.ncomp; i.hsamp = s.hmax; i.vsamp = s.vmax; i.restart_interval = s.restart;
    i.entropy_offset = s.ecs_off; i.entropy_length = s.ecs_len; i.reason = s.reason;
    return i;
}

}  // namespace jpegdec
}  // namespace rebvo
