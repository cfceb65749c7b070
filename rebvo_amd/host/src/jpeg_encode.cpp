// jpeg_encode.cpp — see rebvo/jpeg_encode.h.  libjpeg's baseline encoder at its defaults, restated in integers: jccolor.c (16.16 fixed
// point), jcsample.c (h2v2 with the alternating bias), jccoefct.c (dummy blocks), jfdctint.c, jcdctmgr.c (the quantiser's rounding),
// jchuff.c (one interleaved scan, byte stuffing).  The CPU yardstick of the device encoder (edgehip_jpeg_encode).
#include "rebvo/jpeg_encode.h"

#include <algorithm>

namespace rebvo {
namespace jpeg {

namespace {

inline int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint.c, CONST_BITS = 13, PASS1_BITS = 2: one 1-D pass over eight values; pass 1 (rows) leaves the results scaled up by 4,
// pass 2 (columns) removes that again
template <bool kPass1>
inline void fdct8(int d[8]) {
    const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    constexpr int n = kPass1 ? 11 : 15;
    d[0] = kPass1 ? (tmp10 + tmp11) * 4 : descale(tmp10 + tmp11, 2);
    d[4] = kPass1 ? (tmp10 - tmp11) * 4 : descale(tmp10 - tmp11, 2);
    int z1 = (tmp12 + tmp13) * 4433;
    d[2] = descale(z1 + tmp13 * 6270, n);
    d[6] = descale(z1 + tmp12 * -15137, n);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * 9633;
    const int t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
    z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
    z3 += z5; z4 += z5;
    d[7] = descale(t4 + z1 + z3, n);
    d[5] = descale(t5 + z2 + z4, n);
    d[3] = descale(t6 + z2 + z3, n);
    d[1] = descale(t7 + z1 + z4, n);
}

// 8x8 samples (0..255) -> quantised coefficients in zig-zag order
void block_coefs(const uint8_t s[64], const uint8_t q[64], int out[64]) {
    int v[64];
    for (int i = 0; i < 64; i++) v[i] = (int)s[i] - 128;
    for (int r = 0; r < 8; r++) fdct8<true>(v + r * 8);
    for (int c = 0; c < 8; c++) {
        int col[8];
        for (int r = 0; r < 8; r++) col[r] = v[r * 8 + c];
        fdct8<false>(col);
        for (int r = 0; r < 8; r++) v[r * 8 + c] = col[r];
    }
    for (int k = 0; k < 64; k++) {
        const int nat = kZigzag[k], d = 8 * q[nat], c = v[nat];
        out[k] = c >= 0 ? (c + d / 2) / d : -((-c + d / 2) / d);
    }
}

struct BitWriter {
    std::vector<uint8_t> &o;
    uint64_t acc = 0;
    int n = 0;
    int64_t stuffed = 0;
    void byte(uint8_t b) { o.push_back(b); if (b == 0xFF) { o.push_back(0); stuffed++; } }
    void put(uint32_t code, int len) {
        acc = (acc << len) | code;
        n += len;
        while (n >= 8) { byte((uint8_t)(acc >> (n - 8))); n -= 8; }
    }
    void finish() { if (n) put((1u << (8 - n)) - 1, 8 - n); }
};

inline int category(int a) { int n = 0; while (a) { n++; a >>= 1; } return n; }   // bits of |v|

}  // namespace

bool encode(const uint8_t *rgb, int w, int h, int quality, const char *comment, size_t comment_len, std::vector<uint8_t> &out, Stats *stats) {
    if (!rgb || w < 1 || h < 1 || w > 65535 || h > 65535 || quality < 1 || quality > 100 || comment_len > 65533) return false;
    const int mw = (w + 15) / 16, mh = (h + 15) / 16, bw = (w + 7) / 8, bh = (h + 7) / 8, ch = (h + 1) / 2;
    uint8_t q[2][64];
    quant_tables(quality, q);
    HuffCodes hc;
    huff_codes(&hc);
    out = header(w, h, quality, comment, comment_len);
    Stats st = {};
    BitWriter bwr{out};

    auto px = [&](int x, int y) { return rgb + ((size_t)std::min(y, h - 1) * w + std::min(x, w - 1)) * 3; };
    auto luma = [&](int x, int y) { const uint8_t *p = px(x, y); return (uint8_t)((19595 * p[0] + 38470 * p[1] + 7471 * p[2] + 32768) >> 16); };
    // chroma sample (cx, cy) of plane c (0 Cb, 1 Cr): columns replicated before the downsampling, rows (beyond one for an odd height) after it
    auto chroma = [&](int c, int cx, int cy) {
        cy = std::min(cy, ch - 1);
        int sum = 0;
        for (int dy = 0; dy < 2; dy++)
            for (int dx = 0; dx < 2; dx++) {
                const uint8_t *p = px(2 * cx + dx, 2 * cy + dy);
                sum += c == 0 ? (-11059 * p[0] - 21709 * p[1] + 32768 * p[2] + (128 << 16) + 32767) >> 16
                              : (32768 * p[0] - 27439 * p[1] - 5329 * p[2] + (128 << 16) + 32767) >> 16;
            }
        return (uint8_t)((sum + 1 + (cx & 1)) >> 2);
    };
    auto code_block = [&](const int *cf, int tbl, int &pred) {
        const int diff = cf[0] - pred;
        pred = cf[0];
        int nb = category(diff < 0 ? -diff : diff);
        st.max_dc_cat = std::max<int64_t>(st.max_dc_cat, nb);
        bwr.put(hc.dc[tbl][nb] & 0xFFFF, (int)(hc.dc[tbl][nb] >> 16));
        if (nb) bwr.put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1), nb);
        int run = 0;
        for (int k = 1; k < 64; k++) {
            const int v = cf[k];
            if (!v) { run++; continue; }
            for (; run > 15; run -= 16) { bwr.put(hc.ac[tbl][0xF0] & 0xFFFF, (int)(hc.ac[tbl][0xF0] >> 16)); st.zrl++; }
            nb = category(v < 0 ? -v : v);
            st.max_ac_cat = std::max<int64_t>(st.max_ac_cat, nb);
            const uint32_t c = hc.ac[tbl][(run << 4) | nb];
            bwr.put(c & 0xFFFF, (int)(c >> 16));
            bwr.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << nb) - 1), nb);
            run = 0;
        }
        if (run) bwr.put(hc.ac[tbl][0] & 0xFFFF, (int)(hc.ac[tbl][0] >> 16));
        else st.no_eob++;
        st.blocks++;
    };

    int pred[3] = {0, 0, 0};
    uint8_t s[64];
    int cf[64], last[64] = {0};
    for (int my = 0; my < mh; my++)
        for (int mx = 0; mx < mw; mx++) {
            for (int j = 0; j < 4; j++) {
                const int bx = mx * 2 + (j & 1), by = my * 2 + (j >> 1);
                if (bx < bw && by < bh) {
                    for (int i = 0; i < 64; i++) s[i] = luma(bx * 8 + (i & 7), by * 8 + (i >> 3));
                    block_coefs(s, q[0], cf);
                } else {   // jccoefct.c's dummy block: the DC of the block coded before it, no AC
                    for (int i = 1; i < 64; i++) cf[i] = 0;
                    cf[0] = last[0];
                    if (bx >= bw) st.dummy_right++;
                    if (by >= bh) st.dummy_bottom++;
                }
                memcpy(last, cf, sizeof cf);
                code_block(cf, 0, pred[0]);
            }
            for (int c = 0; c < 2; c++) {
                for (int i = 0; i < 64; i++) s[i] = chroma(c, mx * 8 + (i & 7), my * 8 + (i >> 3));
                block_coefs(s, q[1], cf);
                code_block(cf, 1, pred[1 + c]);
            }
        }
    bwr.finish();
    st.stuffed = bwr.stuffed;
    out.push_back(0xFF);
    out.push_back(0xD9);
    if (stats) *stats = st;
    return true;
}

}  // namespace jpeg
}  // namespace rebvo

extern "C" long long rebvo_encode_jpeg(const unsigned char *rgb, int w, int h, int quality, const char *comment, unsigned char *out, long long cap,
                                       long long *stats) {
    std::vector<uint8_t> o;
    rebvo::jpeg::Stats st;
    static_assert(sizeof(rebvo::jpeg::Stats) == 8 * sizeof(long long), "eight int64");
    if (!rebvo::jpeg::encode(rgb, w, h, quality, comment, comment ? strlen(comment) : 0, o, &st)) return -1;
    if (out && (long long)o.size() <= cap) memcpy(out, o.data(), o.size());
    if (stats) memcpy(stats, &st, sizeof st);
    return (long long)o.size();
}
