// jpeg_pixels.h — the pixel rules of the device JPEG decoder, in integers only and as jpeg_reader.cpp states them (libjpeg's
// jpeg_idct_islow, h2v1 / h2v2 fancy upsampling with its edge rules, ycc_rgb_convert), one value at a time so that a kernel thread
// (jpeg_decode.hip) and a plain loop (rebvo_amd/host/src/jpeg_decode.cpp) run the same code.
#pragma once
#include "rebvo/jpeg_decode.h"

namespace rebvo {
namespace jpegdec {

REBVO_JD_HD inline int px_descale(long long x, int n) { return (int)((x + ((long long)1 << (n - 1))) >> n); }
REBVO_JD_HD inline int px_clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// jidctint.c's 1-D kernel (CONST_BITS 13): in[8] -> the eight sums before descaling, out[i] and out[7 - i] from the same pair
REBVO_JD_HD inline void px_idct8(const int in[8], long long out[8]) {
    long long z2 = in[2], z3 = in[6];
    long long z1 = (z2 + z3) * 4433;
    long long tmp2 = z1 + z3 * (-15137);
    long long tmp3 = z1 + z2 * 6270;
    long long tmp0 = ((long long)in[0] + in[4]) * (1 << 13);
    long long tmp1 = ((long long)in[0] - in[4]) * (1 << 13);
    const long long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    long long z4 = tmp1 + tmp3;
    const long long z5 = (z3 + z4) * 9633;
    tmp0 *= 2446; tmp1 *= 16819; tmp2 *= 25172; tmp3 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    out[0] = tmp10 + tmp3; out[7] = tmp10 - tmp3;
    out[1] = tmp11 + tmp2; out[6] = tmp11 - tmp2;
    out[2] = tmp12 + tmp1; out[5] = tmp12 - tmp1;
    out[3] = tmp13 + tmp0; out[4] = tmp13 - tmp0;
}
// pass 1, one column of dequantised coefficients -> one column of the workspace (scaled up by 2^PASS1_BITS = 4)
REBVO_JD_HD inline void px_idct_col(const int in[8], int ws[8]) {
    if (in[1] == 0 && in[2] == 0 && in[3] == 0 && in[4] == 0 && in[5] == 0 && in[6] == 0 && in[7] == 0) {
        const int dc = (int)((long long)in[0] * 4);
        for (int r = 0; r < 8; r++) ws[r] = dc;
        return;
    }
    long long o[8];
    px_idct8(in, o);
    for (int r = 0; r < 8; r++) ws[r] = px_descale(o[r], 13 - 2);
}
// pass 2, one row of the workspace -> eight samples
REBVO_JD_HD inline void px_idct_row(const int ws[8], uint8_t out[8]) {
    long long o[8];
    px_idct8(ws, o);
    for (int c = 0; c < 8; c++) out[c] = (uint8_t)px_clamp8(px_descale(o[c], 13 + 2 + 3) + 128);
}

// The component's value at image position (x, y): its plane [hblocks * 8][stride] holds cw x ch true samples, (hx, vx) is what one
// sample covers — (1, 1), (2, 1) h2v1 or (2, 2) h2v2.  The image's first and last sample rows repeat as context rows (jdmainct.c), the
// first and last columns follow jdsample.c's special cases.
REBVO_JD_HD inline int px_sample(const uint8_t *plane, int stride, int cw, int ch, int hx, int vx, int x, int y) {
    if (hx == 1) return plane[(size_t)y * stride + x];
    const int c = x >> 1;
    if (vx == 1) {
        const uint8_t *in = plane + (size_t)y * stride;
        if (x & 1) return c == cw - 1 ? in[c] : (in[c] * 3 + in[c + 1] + 2) >> 2;
        return c == 0 ? in[c] : (in[c] * 3 + in[c - 1] + 1) >> 2;
    }
    const int r = y >> 1;
    int rf = (y & 1) ? r + 1 : r - 1;
    rf = rf < 0 ? 0 : (rf >= ch ? ch - 1 : rf);
    const uint8_t *in0 = plane + (size_t)r * stride, *in1 = plane + (size_t)rf * stride;
    const int cur = in0[c] * 3 + in1[c];
    if (x & 1) {
        if (c == cw - 1) return (cur * 4 + 7) >> 4;
        return (cur * 3 + in0[c + 1] * 3 + in1[c + 1] + 7) >> 4;
    }
    if (c == 0) return (cur * 4 + 8) >> 4;
    return (cur * 3 + in0[c - 1] * 3 + in1[c - 1] + 8) >> 4;
}

// ycc_rgb_convert: 16.16 fixed point, ONE_HALF rounding, arithmetic right shifts -> r | g << 8 | b << 16
REBVO_JD_HD inline uint32_t px_ycc_rgb(int Y, int cb, int cr) {
    const int r = Y + ((91881 * (cr - 128) + 32768) >> 16);
    const int g = Y + ((-22554 * (cb - 128) + 32768 + -46802 * (cr - 128)) >> 16);
    const int b = Y + ((116130 * (cb - 128) + 32768) >> 16);
    return (uint32_t)px_clamp8(r) | ((uint32_t)px_clamp8(g) << 8) | ((uint32_t)px_clamp8(b) << 16);
}

// the pixel (x, y) of stream s from its sample planes (component ci's plane at samples + block_base * 64, stride wblocks * 8)
REBVO_JD_HD inline uint32_t px_pixel(const Stream &s, const uint8_t *samples, int x, int y) {
    int v[3] = {0, 0, 0};
    for (int ci = 0; ci < s.ncomp; ci++) {
        const Comp &c = s.comp[ci];
        v[ci] = px_sample(samples + (size_t)c.block_base * 64, c.wblocks * 8, c.cw, c.ch, s.hmax / c.h, s.vmax / c.v, x, y);
    }
    return s.ncomp == 1 ? (uint32_t)v[0] * 0x010101u : px_ycc_rgb(v[0], v[1], v[2]);
}

}  // namespace jpegdec
}  // namespace rebvo
