// jpeg_encode.h — the reference's MJPEGEncoder (src/VideoLib/video_mjpeg.cpp:63-74: gdImageJpegPtr, i.e. libjpeg with jpeg_set_defaults and
// jpeg_set_quality(q, TRUE)) as a plain integer rule: baseline, 8 bit, YCbCr 4:2:0, the Annex-K Huffman tables, the islow DCT, no restart
// markers.  This header holds what the host encoder (src/jpeg_encode.cpp) and the device encoder (csrc/jpeg_encode.hip) share: the
// tables, the header and the size bound.  The stream is libjpeg's byte for byte; gd's own decoration (its COM text, and in newer gd a
// density in APP0) could not be compared because no libgd was at hand: the comment is the caller's, the density 1x1 without units.
#ifndef REBVO_AMD_HOST_JPEG_ENCODE_H
#define REBVO_AMD_HOST_JPEG_ENCODE_H

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace rebvo {
namespace jpeg {

constexpr int kHeaderBytes = 623;   // SOI .. SOS without a COM segment

// position in the zig-zag sequence -> natural (row-major) index
constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// Annex K.1, natural order
constexpr uint8_t kBaseQuant[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// Annex K.3: code counts per length 1..16 and the symbols, for DC luma / DC chroma / AC luma / AC chroma
constexpr uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

// jpeg_set_quality(q, TRUE): Annex K scaled by jpeg_quality_scaling, clamped to 1..255 (baseline); natural order
inline void quant_tables(int quality, uint8_t q[2][64]) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; t++)
        for (int i = 0; i < 64; i++) {
            const int v = (kBaseQuant[t][i] * scale + 50) / 100;
            q[t][i] = (uint8_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
}

// Every symbol's code as (length << 16) | code, 0 for a symbol the table lacks (jchuff.c, jpeg_make_c_derived_tbl).
// [0] DC luma, [1] DC chroma, [2] AC luma, [3] AC chroma
struct HuffCodes { uint32_t dc[2][12]; uint32_t ac[2][256]; };
inline void huff_codes(HuffCodes *h) {
    memset(h, 0, sizeof *h);
    for (int t = 0; t < 4; t++) {
        const uint8_t *bits = t < 2 ? kDcBits[t] : kAcBits[t - 2], *vals = t < 2 ? kDcVals : kAcVals[t - 2];
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; len++) {
            for (int i = 0; i < bits[len - 1]; i++, k++, code++) (t < 2 ? h->dc[t] : h->ac[t - 2])[vals[k]] = ((uint32_t)len << 16) | code;
            code <<= 1;
        }
    }
}

// SOI, APP0 (JFIF 1.01, no units, 1x1), [COM with the caller's text, where jpeg_write_marker puts it], DQT 0, DQT 1, SOF0, four DHT, SOS
inline std::vector<uint8_t> header(int w, int h, int quality, const char *comment, size_t comment_len) {
    std::vector<uint8_t> o;
    auto put = [&o](std::initializer_list<int> l) { for (int v : l) o.push_back((uint8_t)v); };
    put({0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    if (comment && comment_len > 0) {
        put({0xFF, 0xFE, (int)((comment_len + 2) >> 8), (int)((comment_len + 2) & 0xFF)});
        o.insert(o.end(), comment, comment + comment_len);
    }
    uint8_t q[2][64];
    quant_tables(quality, q);
    for (int t = 0; t < 2; t++) {
        put({0xFF, 0xDB, 0, 67, t});
        for (int i = 0; i < 64; i++) o.push_back(q[t][kZigzag[i]]);
    }
    put({0xFF, 0xC0, 0, 17, 8, h >> 8, h & 0xFF, w >> 8, w & 0xFF, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (int t = 0; t < 2; t++)
        for (int ac = 0; ac < 2; ac++) {
            const uint8_t *bits = ac ? kAcBits[t] : kDcBits[t], *vals = ac ? kAcVals[t] : kDcVals;
            const int n = ac ? 162 : 12;
            put({0xFF, 0xC4, (19 + n) >> 8, (19 + n) & 0xFF, (ac << 4) | t});
            o.insert(o.end(), bits, bits + 16);
            o.insert(o.end(), vals, vals + n);
        }
    put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    return o;
}

// No frame is longer: header, COM segment, every block at its longest code (a DC code of 11 bits with 11 more, 63 AC codes of 16 bits
// with 10 more), every data byte stuffed, EOI.
inline size_t bound(int w, int h, size_t comment_len) {
    const size_t nblocks = (size_t)6 * ((w + 15) / 16) * ((h + 15) / 16);
    return kHeaderBytes + (comment_len ? comment_len + 4 : 0) + 2 * ((nblocks * (22 + 63 * 26) + 7) / 8) + 2;
}

// what the stream of one image exercises (the fixture tool asserts these populations, the CPU test recomputes them)
struct Stats {
    int64_t stuffed;        // FF 00 pairs in the entropy-coded data
    int64_t zrl;            // ZRL symbols (0xF0)
    int64_t no_eob;         // blocks whose coefficient 63 is non-zero
    int64_t max_dc_cat;     // largest DC difference category
    int64_t max_ac_cat;     // largest AC category
    int64_t dummy_right;    // luma blocks right of the last block column
    int64_t dummy_bottom;   // luma blocks below the last block row
    int64_t blocks;         // blocks coded, dummies included
};

// RGB24, w x h >= 1 x 1, quality 1..100, comment may be null; false for arguments outside that (w, h <= 65535, comment <= 65533 bytes)
bool encode(const uint8_t *rgb, int w, int h, int quality, const char *comment, size_t comment_len, std::vector<uint8_t> &out, Stats *stats = nullptr);

}  // namespace jpeg
}  // namespace rebvo

extern "C" {
/* flat view (tests, tools): the stream's length, written to `out` when it fits in `cap` (out may be null to ask for the length); -1 for bad
 * arguments.  `comment` is a C string or null.  `stats`: eight int64 in the order of rebvo::jpeg::Stats, or null. */
long long rebvo_encode_jpeg(const unsigned char *rgb, int w, int h, int quality, const char *comment, unsigned char *out, long long cap,
                            long long *stats);
/* the library's own reader (jpeg_reader.cpp) on a stream in memory: w, h and, when 3 * w * h <= cap, the RGB24 pixels; -1 when it cannot
 * be decoded */
int rebvo_decode_jpeg(const unsigned char *data, long long len, unsigned char *rgb, long long cap, int *w, int *h);
}
#endif
