// jpeg_encode.hip — the reference's MJPEGEncoder on the device: what its output thread does with a finished frame before it sends or saves
// it (src/rebvo/rebvo_third_t.cpp:184-257 -> src/VideoLib/video_mjpeg.cpp:63-74 -> gdImageJpegPtr -> libjpeg at its defaults), for every
// sequence of a slot in one launch.  The rule is rebvo/jpeg_encode.h's (all integer, libjpeg's bytes); the host encoder there is the
// yardstick.
//
// One workgroup per image walks the image's MCUs in scan order, kJpSegMcu at a time (a segment: 72 blocks, whatever the image's width, so
// nothing depends on the geometry).  Per segment, with all 256 threads:
//   fetch     the segment's pixels through the slot's accessors (RGB24, 8-bit mono, a bound pool frame, the undistortion map), colour
//             conversion and h2v2 downsampling into 8x8 sample blocks in LDS
//   DCT       jfdctint's row pass (one thread per block row), its column pass with the quantiser (one thread per block column); the
//             quantised coefficients stay in LDS, in zig-zag order, 16 bit
//   lengths   one thread per block: the block's code length from its own coefficients and the DC of the block before it; a workgroup
//             scan gives every block its bit offset
//   bits      the same threads write their codes at those offsets, a 32-bit word at a time, with atomicOr on zeroed LDS words
//   stuffing  moves bytes: every thread counts the FF bytes of its run of whole bytes, a second scan gives the shifted positions
//   store     the whole 16-byte words of the result leave through flush_words (pack_flush.h); the up to 15 bytes behind them and the up to
//             7 bits that do not fill a byte yet are carried into the next segment, as are the three DC predictors
// The carries stay inside the workgroup: no workgroup waits for another one, and the bytes of an image do not depend on the batch it is in.
#include "ctx.h"
#include "pack_flush.h"
#include "stage_a_dev.h"
#include "rebvo/jpeg_encode.h"

#include <algorithm>
#include <vector>

namespace edgehip {

constexpr int kJpThreads = 256;
constexpr int kJpSegMcu = 12;                                  // MCUs per segment
constexpr int kJpSegBlocks = 6 * kJpSegMcu;
constexpr int kJpStride = 66;                                  // int16 per block in LDS: 33 dwords, so that a thread per block meets no bank twice
constexpr int kJpBlockBits = 22 + 63 * 26;                     // the longest code of one block (rebvo::jpeg::bound)
constexpr int kJpSegBits = 7 + kJpSegBlocks * kJpBlockBits;    // with the bits carried in
constexpr int kJpBitWords = (kJpSegBits + 31) / 32 + 1;
constexpr int kJpSegBytes = (kJpSegBits + 7) / 8;
constexpr int kJpImgBytes = (15 + 2 * kJpSegBytes + 2 + 15) & ~15;   // carried bytes, every byte stuffed, EOI
constexpr int kJpPass2 = (kJpSegBlocks * 8 + kJpThreads - 1) / kJpThreads;   // block columns per thread

struct JpegTables {
    uint32_t recip[2][64];   // natural order: floor(2^32 / (8 q)) + 1 — __umulhi(n, recip) == n / (8 q) for every n the DCT can give
    uint16_t half[2][64];    // 4 q
    uint8_t zzpos[64];       // natural index -> position in the zig-zag sequence
    uint32_t dc[2][12];      // (length << 16) | code
    uint32_t ac[2][256];
};
static_assert(sizeof(JpegTables) % 16 == 0, "copied and carved in 16-byte words");

struct JpegArgs {
    const uint8_t *rgb;          // RGB24 frames (image i at (fidx ? fidx[i] : i) * n * 3), or null
    const uint8_t *grey8;        // 8-bit mono frames (same indexing, n bytes each), or null
    const int32_t *fidx;         // frame index inside a bound pool, or null
    const int32_t *und_base;     // [n] / [n] the undistortion map (stage_a_dev.h), or null
    const uint4 *und_iw;
    const JpegTables *tab;
    const uint8_t *hdr;          // SOI .. SOS, hlen bytes (16-byte aligned)
    uint8_t *out;                // image i's region at i * stride (16-byte aligned), cap bytes of it may be written
    edgehip_jpeg_size *sizes;    // [images]
    const uint8_t *mask;         // [images] or null: images with a zero byte are left alone
    const int32_t *req;          // [images] or null: image i is the frame of sequence req[i] (edgehip_jpeg_export: regions by request, not by sequence)
    size_t stride;
    uint32_t cap;
    int hlen, w, h, n;
};

// one pixel as r | g << 8 | b << 16, whatever the slot holds
__device__ __forceinline__ uint32_t jp_pixel(const JpegArgs &a, const uint8_t *__restrict__ frame, int x, int y) {
    const int pix = y * a.w + x;
    if (a.und_base) {   // image_undistort::undistort<true>: what PipeBuffer::imgc holds with UseUndistort
        if (!a.grey8) {
            const uchar3 c = undist_rgb(frame, a.und_base[pix], a.und_iw[pix], a.w, a.n);
            return (uint32_t)c.x | ((uint32_t)c.y << 8) | ((uint32_t)c.z << 16);
        }
        // a mono frame: the same four taps on r = g = b = v (a tap of weight 0 may lie outside the frame)
        const int base = a.und_base[pix];
        const uint4 iw = a.und_iw[pix];
        const int at[4] = {base, base + 1, base + a.w, base + a.w + 1};
        const uint32_t wt[4] = {iw.x, iw.y, iw.z, iw.w};
        int s = 0;
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (wt[i] != 0 && at[i] >= 0 && at[i] < a.n) s += (int)wt[i] * (int)frame[at[i]];
        return (uint32_t)((s >> 16) & 0xFF) * 0x010101u;
    }
    if (a.grey8) return (uint32_t)frame[pix] * 0x010101u;
    const uint8_t *p = frame + (size_t)pix * 3;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}
// jccolor.c, 16.16 fixed point
__device__ __forceinline__ int jp_y(uint32_t p) { return (int)((19595u * (p & 0xFF) + 38470u * ((p >> 8) & 0xFF) + 7471u * (p >> 16) + 32768u) >> 16); }
__device__ __forceinline__ int jp_cb(uint32_t p) {
    return (-11059 * (int)(p & 0xFF) - 21709 * (int)((p >> 8) & 0xFF) + 32768 * (int)(p >> 16) + (128 << 16) + 32767) >> 16;
}
__device__ __forceinline__ int jp_cr(uint32_t p) {
    return (32768 * (int)(p & 0xFF) - 27439 * (int)((p >> 8) & 0xFF) - 5329 * (int)(p >> 16) + (128 << 16) + 32767) >> 16;
}

__device__ __forceinline__ int jp_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
// jfdctint.c (CONST_BITS 13, PASS1_BITS 2): the row pass leaves its results scaled up by 4, the column pass takes that out again
template <bool kPass1>
__device__ __forceinline__ void jp_fdct8(int d[8]) {
    const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    constexpr int n = kPass1 ? 11 : 15;
    d[0] = kPass1 ? (tmp10 + tmp11) * 4 : jp_descale(tmp10 + tmp11, 2);
    d[4] = kPass1 ? (tmp10 - tmp11) * 4 : jp_descale(tmp10 - tmp11, 2);
    int z1 = (tmp12 + tmp13) * 4433;
    d[2] = jp_descale(z1 + tmp13 * 6270, n);
    d[6] = jp_descale(z1 + tmp12 * -15137, n);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * 9633;
    const int t4 = tmp4 * 2446, t5 = tmp5 * 16819, t6 = tmp6 * 25172, t7 = tmp7 * 12299;
    z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
    z3 += z5; z4 += z5;
    d[7] = jp_descale(t4 + z1 + z3, n);
    d[5] = jp_descale(t5 + z2 + z4, n);
    d[3] = jp_descale(t6 + z2 + z3, n);
    d[1] = jp_descale(t7 + z1 + z4, n);
}

// exclusive scan of one value per thread over the workgroup, the total to every thread; ws: kJpThreads / 64 + 1 ints of LDS, free again on return
__device__ __forceinline__ int jp_exscan(int v, int *ws, int &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    int before = 0, sum = 0;
#pragma unroll
    for (int i = 0; i < kJpThreads / 64; i++) {
        const int t = ws[i];
        if (i < wave) before += t;
        sum += t;
    }
    __syncthreads();
    total = sum;
    return before + inc - v;
}

// the block whose quantised DC luma block j of an MCU carries: itself, or for jccoefct.c's dummy blocks (right of the last block column,
// below the last block row) the block coded before it, which may be a dummy too
__device__ __forceinline__ int jp_dc_src(int j, bool right, bool bottom) {
    if (j == 1) return right ? 0 : 1;
    if (j == 2) return bottom ? (right ? 0 : 1) : 2;
    if (j == 3) return bottom ? (right ? 0 : 1) : (right ? 2 : 3);
    return j;
}
__device__ __forceinline__ int jp_bits_of(int v) { return v ? 32 - __clz(v < 0 ? -v : v) : 0; }

__global__ __launch_bounds__(kJpThreads) void k_jpeg_encode(JpegArgs a) {
    __shared__ __align__(16) int16_t coef[kJpSegBlocks * kJpStride];
    __shared__ __align__(16) uint32_t bits[kJpBitWords];
    __shared__ __align__(16) uint8_t img[kJpImgBytes];
    __shared__ __align__(16) JpegTables tab;
    __shared__ int ws[kJpThreads / 64 + 1];
    const int img_i = blockIdx.x, seq = a.req ? a.req[img_i] : img_i, tid = threadIdx.x;
    if (a.mask && !a.mask[seq]) return;

    for (int i = tid; i < (int)(sizeof(JpegTables) / 4); i += kJpThreads) reinterpret_cast<uint32_t *>(&tab)[i] = reinterpret_cast<const uint32_t *>(a.tab)[i];
    uint8_t *region = a.out + (size_t)img_i * a.stride;
    // the header: its whole words straight to the region (cap >= hlen + 2), the rest waits in img for the first data bytes
    for (int t = tid; t < (a.hlen >> 4); t += kJpThreads) reinterpret_cast<uint4 *>(region)[t] = reinterpret_cast<const uint4 *>(a.hdr)[t];
    if (tid < (a.hlen & 15)) img[tid] = a.hdr[(a.hlen & ~15) + tid];

    const size_t fi = a.fidx ? (size_t)a.fidx[seq] : (size_t)seq;
    const uint8_t *frame = a.grey8 ? a.grey8 + fi * (size_t)a.n : a.rgb + fi * (size_t)a.n * 3;
    const int w = a.w, h = a.h, mw = (w + 15) >> 4, mh = (h + 15) >> 4, bw = (w + 7) >> 3, bh = (h + 7) >> 3, ch = (h + 1) >> 1;
    const int nmcu = mw * mh;

    uint32_t pos = (uint32_t)a.hlen;       // bytes of the stream so far (the true count, also past cap)
    int pend = a.hlen & 15;                // of them, waiting at the front of img for their 16-byte word to fill
    int cbits = 0;                         // bits carried in (< 8) and their value
    uint32_t cval = 0;
    int pdc0 = 0, pdc1 = 0, pdc2 = 0;      // DC predictors: Y, Cb, Cr
    __syncthreads();

    for (int m0 = 0; m0 < nmcu; m0 += kJpSegMcu) {
        const int nm = min(kJpSegMcu, nmcu - m0), nblk = nm * 6;
        const bool last = m0 + kJpSegMcu >= nmcu;

        // ---- fetch: one thread per 2x2 pixels, four luma samples and one sample of either chroma plane
        for (int q = tid; q < nm * 64; q += kJpThreads) {
            const int ml = q >> 6, m = m0 + ml, my = m / mw, mx = m - my * mw, qy = (q >> 3) & 7, qx = q & 7;
            const int x0 = min(mx * 16 + 2 * qx, w - 1), x1 = min(mx * 16 + 2 * qx + 1, w - 1);
            int y0 = min(my * 16 + 2 * qy, h - 1), y1 = min(my * 16 + 2 * qy + 1, h - 1);
            uint32_t p[4] = {jp_pixel(a, frame, x0, y0), jp_pixel(a, frame, x1, y0), jp_pixel(a, frame, x0, y1), jp_pixel(a, frame, x1, y1)};
            int16_t *yb = coef + (ml * 6 + (qy >> 2) * 2 + (qx >> 2)) * kJpStride + ((2 * qy) & 7) * 8 + ((2 * qx) & 7);
            yb[0] = (int16_t)(jp_y(p[0]) - 128); yb[1] = (int16_t)(jp_y(p[1]) - 128);
            yb[8] = (int16_t)(jp_y(p[2]) - 128); yb[9] = (int16_t)(jp_y(p[3]) - 128);
            // chroma rows are replicated AFTER the downsampling (an odd height's last row once before it): below the last chroma row the
            // sample is that row's, not the mean of two replicated luma rows
            const int cy = my * 8 + qy;
            if (cy > ch - 1) {
                y0 = 2 * (ch - 1); y1 = min(y0 + 1, h - 1);
                p[0] = jp_pixel(a, frame, x0, y0); p[1] = jp_pixel(a, frame, x1, y0); p[2] = jp_pixel(a, frame, x0, y1); p[3] = jp_pixel(a, frame, x1, y1);
            }
            const int bias = 1 + (qx & 1);   // jcsample.c h2v2: 1, 2, 1, 2, ... along the output row
            const int cb = (jp_cb(p[0]) + jp_cb(p[1]) + jp_cb(p[2]) + jp_cb(p[3]) + bias) >> 2;
            const int cr = (jp_cr(p[0]) + jp_cr(p[1]) + jp_cr(p[2]) + jp_cr(p[3]) + bias) >> 2;
            coef[(ml * 6 + 4) * kJpStride + qy * 8 + qx] = (int16_t)(cb - 128);
            coef[(ml * 6 + 5) * kJpStride + qy * 8 + qx] = (int16_t)(cr - 128);
        }
        __syncthreads();

        // ---- DCT rows, in place
        for (int it = tid; it < nblk * 8; it += kJpThreads) {
            int16_t *row = coef + (it >> 3) * kJpStride + (it & 7) * 8;
            int d[8];
#pragma unroll
            for (int i = 0; i < 8; i++) d[i] = row[i];
            jp_fdct8<true>(d);
#pragma unroll
            for (int i = 0; i < 8; i++) row[i] = (int16_t)d[i];
        }
        __syncthreads();

        // ---- DCT columns and the quantiser: every column is read before any coefficient goes to its zig-zag place
        int col[kJpPass2][8];
#pragma unroll
        for (int k = 0; k < kJpPass2; k++) {
            const int it = tid + k * kJpThreads;
            if (it < nblk * 8) {
                const int16_t *c0 = coef + (it >> 3) * kJpStride + (it & 7);
#pragma unroll
                for (int r = 0; r < 8; r++) col[k][r] = c0[r * 8];
                jp_fdct8<false>(col[k]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kJpPass2; k++) {
            const int it = tid + k * kJpThreads;
            if (it < nblk * 8) {
                const int blk = it >> 3, c = it & 7, ml = blk / 6, j = blk - ml * 6, m = m0 + ml, my = m / mw, mx = m - my * mw;
                const int t = j >= 4 ? 1 : 0;
                const bool dummy = j < 4 && (mx * 2 + (j & 1) >= bw || my * 2 + (j >> 1) >= bh);
#pragma unroll
                for (int r = 0; r < 8; r++) {
                    const int nat = r * 8 + c, v = col[k][r];
                    const int qv = (int)__umulhi((uint32_t)((v < 0 ? -v : v) + tab.half[t][nat]), tab.recip[t][nat]);
                    coef[blk * kJpStride + tab.zzpos[nat]] = dummy ? (int16_t)0 : (int16_t)(v < 0 ? -qv : qv);
                }
            }
        }
        __syncthreads();

        // ---- code lengths: one thread per block
        int len = 0, diff = 0, tbl = 0;
        bool dummy = false;
        if (tid < nblk) {
            const int ml = tid / 6, j = tid - ml * 6, m = m0 + ml, my = m / mw, mx = m - my * mw;
            const bool right = mx * 2 + 1 >= bw, bottom = my * 2 + 1 >= bh;
            tbl = j >= 4 ? 1 : 0;
            dummy = j < 4 && jp_dc_src(j, right, bottom) != j;
            const int dc = coef[(ml * 6 + jp_dc_src(j, right, bottom)) * kJpStride];
            int pred;
            if (j >= 1 && j <= 3) {
                pred = coef[(ml * 6 + jp_dc_src(j - 1, right, bottom)) * kJpStride];
            } else if (ml == 0) {
                pred = j == 0 ? pdc0 : (j == 4 ? pdc1 : pdc2);
            } else if (j == 0) {   // the last luma block of the MCU before
                const int pm = m - 1, pmy = pm / mw, pmx = pm - pmy * mw;
                pred = coef[((ml - 1) * 6 + jp_dc_src(3, pmx * 2 + 1 >= bw, pmy * 2 + 1 >= bh)) * kJpStride];
            } else {
                pred = coef[((ml - 1) * 6 + j) * kJpStride];
            }
            diff = dc - pred;
            const int nb = jp_bits_of(diff);
            len = (int)(tab.dc[tbl][nb] >> 16) + nb;
            const int eob = (int)(tab.ac[tbl][0] >> 16), zrl = (int)(tab.ac[tbl][0xF0] >> 16);
            if (dummy) {
                len += eob;
            } else {
                const uint32_t *cw = reinterpret_cast<const uint32_t *>(coef + tid * kJpStride);
                int run = 0;
                for (int kk = 0; kk < 32; kk++) {
                    const uint32_t u = cw[kk];
#pragma unroll
                    for (int s = 0; s < 2; s++) {
                        if (kk == 0 && s == 0) continue;
                        const int v = (int)(int16_t)(s ? u >> 16 : u & 0xFFFF);
                        if (v == 0) { run++; continue; }
                        const int n2 = jp_bits_of(v);
                        len += (run >> 4) * zrl + (int)(tab.ac[tbl][((run & 15) << 4) | n2] >> 16) + n2;
                        run = 0;
                    }
                }
                if (run) len += eob;
            }
        }
        int tbits;
        const int off = jp_exscan(len, ws, tbits);
        // the predictors of the next segment, while this one's coefficients are still there
        {
            const int m = m0 + nm - 1, my = m / mw, mx = m - my * mw;
            pdc0 = coef[((nm - 1) * 6 + jp_dc_src(3, mx * 2 + 1 >= bw, my * 2 + 1 >= bh)) * kJpStride];
            pdc1 = coef[((nm - 1) * 6 + 4) * kJpStride];
            pdc2 = coef[((nm - 1) * 6 + 5) * kJpStride];
        }
        const int tb = cbits + tbits;   // bits in the buffer: the carried ones first
        for (int i = tid; i < ((tb + 31) >> 5) + 1; i += kJpThreads) bits[i] = 0;
        __syncthreads();

        // ---- the codes, at their offsets: most significant bit first, whole 32-bit words at a time
        if (tid == 0 && cbits) atomicOr(&bits[0], cval << (32 - cbits));
        if (tid < nblk) {
            const int p0 = cbits + off;
            int wi = p0 >> 5, nacc = p0 & 31;
            uint64_t acc = 0;
            auto put = [&](uint32_t code, int n) {
                acc = (acc << n) | code;
                nacc += n;
                if (nacc >= 32) {
                    atomicOr(&bits[wi++], (uint32_t)(acc >> (nacc - 32)));
                    nacc -= 32;
                    acc &= (1ull << nacc) - 1;
                }
            };
            {
                const int nb = jp_bits_of(diff);
                const uint32_t c = tab.dc[tbl][nb];
                put(((c & 0xFFFF) << nb) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1)), (int)(c >> 16) + nb);
            }
            const uint32_t eob = tab.ac[tbl][0], zrl = tab.ac[tbl][0xF0];
            int run = 0;
            if (dummy) {
                run = 63;
            } else {
                const uint32_t *cw = reinterpret_cast<const uint32_t *>(coef + tid * kJpStride);
                for (int kk = 0; kk < 32; kk++) {
                    const uint32_t u = cw[kk];
#pragma unroll
                    for (int s = 0; s < 2; s++) {
                        if (kk == 0 && s == 0) continue;
                        const int v = (int)(int16_t)(s ? u >> 16 : u & 0xFFFF);
                        if (v == 0) { run++; continue; }
                        for (; run > 15; run -= 16) put(zrl & 0xFFFF, (int)(zrl >> 16));
                        const int n2 = jp_bits_of(v);
                        const uint32_t c = tab.ac[tbl][(run << 4) | n2];
                        put(((c & 0xFFFF) << n2) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << n2) - 1)), (int)(c >> 16) + n2);
                        run = 0;
                    }
                }
            }
            if (run) put(eob & 0xFFFF, (int)(eob >> 16));
            if (nacc) atomicOr(&bits[wi], (uint32_t)(acc << (32 - nacc)));
        }
        // the last partial byte of the image is filled with 1-bits (they cannot cross a byte, so not a word either)
        if (last && tid == 0 && (tb & 7)) {
            const int pad = 8 - (tb & 7);
            atomicOr(&bits[tb >> 5], ((1u << pad) - 1) << (32 - (tb & 31) - pad));
        }
        __syncthreads();

        // ---- whole bytes out of the bit buffer, FF followed by 00: count, scan, move
        const int nb = last ? (tb + 7) >> 3 : tb >> 3;
        const int ncb = last ? 0 : tb & 7;
        const uint32_t ncv = ncb ? ((bits[nb >> 2] >> (24 - 8 * (nb & 3))) & 0xFF) >> (8 - ncb) : 0;
        const int wpt = (((nb + 3) >> 2) + kJpThreads - 1) / kJpThreads;   // words per thread
        const int i0 = min(tid * wpt * 4, nb), i1 = min(i0 + wpt * 4, nb);
        int nff = 0;
        for (int i = i0; i < i1; i++) nff += ((bits[i >> 2] >> (24 - 8 * (i & 3))) & 0xFF) == 0xFF;
        int tff;
        const int foff = jp_exscan(nff, ws, tff);
        {
            int o = pend + i0 + foff;
            for (int i = i0; i < i1; i++) {
                const uint32_t b = (bits[i >> 2] >> (24 - 8 * (i & 3))) & 0xFF;
                img[o++] = (uint8_t)b;
                if (b == 0xFF) img[o++] = 0;
            }
        }
        int nout = nb + tff;
        if (last) {
            if (tid == 0) { img[pend + nout] = 0xFF; img[pend + nout + 1] = 0xD9; }
            nout += 2;
        }
        __syncthreads();

        // ---- whole 16-byte words to the region, never past cap; what does not fill a word yet moves to the front of img
        const uint32_t w0 = pos - (uint32_t)pend, end = pos + (uint32_t)nout;
        const uint32_t b1 = min(last ? end : end & ~15u, a.cap);
        if (b1 > w0) flush_words<uint8_t, kJpThreads>(img, region, w0, (int)((b1 - w0 + 15) >> 4), w0, b1);
        const int npend = last ? 0 : (int)(end & 15u);
        const int so = (int)((end & ~15u) - w0);
        uint8_t keep = 0;
        if (tid < npend) keep = img[so + tid];
        __syncthreads();
        if (tid < npend) img[tid] = keep;
        pos = end; pend = npend; cbits = ncb; cval = ncv;
        __syncthreads();
    }
    if (tid == 0) {
        edgehip_jpeg_size s;
        s.size = pos;
        s.overflow = pos > a.cap ? 1u : 0u;
        a.sizes[img_i] = s;
    }
}

static void jpeg_tables(int quality, JpegTables *t) {
    uint8_t q[2][64];
    rebvo::jpeg::quant_tables(quality, q);
    rebvo::jpeg::HuffCodes hc;
    rebvo::jpeg::huff_codes(&hc);
    for (int k = 0; k < 2; k++)
        for (int i = 0; i < 64; i++) {
            t->recip[k][i] = (uint32_t)((1ull << 32) / (8u * q[k][i])) + 1;
            t->half[k][i] = (uint16_t)(4 * q[k][i]);
        }
    for (int i = 0; i < 64; i++) t->zzpos[rebvo::jpeg::kZigzag[i]] = (uint8_t)i;
    memcpy(t->dc, hc.dc, sizeof t->dc);
    memcpy(t->ac, hc.ac, sizeof t->ac);
}

}  // namespace edgehip

using namespace edgehip;

struct edgehip_ctx::JpegStore {
    int quality = 0;
    uint32_t cap = 0;
    size_t stride = 0;                 // cap rounded up to 16
    int hlen = 0;
    void *arena = nullptr;             // regions | size records | tables | header | pool indices | select mask
    uint8_t *out = nullptr;
    edgehip_jpeg_size *sizes = nullptr;
    JpegTables *tab = nullptr;
    uint8_t *hdr = nullptr, *mask = nullptr;
    int32_t *fidx = nullptr;           // [nseq] pool indices of a bound slot, for the encode that reads it
    bool masked = false;
    hipEvent_t ev_done = nullptr;      // behind the last encode: uploads into the slot it read wait for it
    hipEvent_t ev_sizes[ExportRing::R] = {};   // edgehip_jpeg_export: the entry's size records have landed in its page-locked row
};

void edgehip::jpeg_free(edgehip_ctx *c) {
    if (!c->jpeg) return;
    (void)hipStreamSynchronize(c->stream);
    if (c->jpeg->arena) (void)hipFree(c->jpeg->arena);
    if (c->jpeg->ev_done) (void)hipEventDestroy(c->jpeg->ev_done);
    // the export ring's entries are sized by this store's cap: tickets still out are dropped with it
    if (c->jpeg_ring.stream) (void)hipStreamSynchronize(c->jpeg_ring.stream);
    for (auto &t : c->jpeg_ring.t) t = ExportRing::Ticket();
    c->jpeg_ring.drop_memory();
    for (hipEvent_t e : c->jpeg->ev_sizes) if (e) (void)hipEventDestroy(e);
    delete c->jpeg;
    c->jpeg = nullptr;
}

uint64_t edgehip_jpeg_bound(int w, int h, uint32_t comment_len) {
    if (w < 1 || h < 1) return 0;
    return rebvo::jpeg::bound(w, h, comment_len);
}

int edgehip_jpeg_enable(edgehip_ctx *c, int quality, uint32_t cap_bytes, const char *comment) {
    EH_ENTER(c);
    if (cap_bytes == 0) { jpeg_free(c); return 0; }
    const size_t clen = comment ? strlen(comment) : 0;
    if (quality < 1 || quality > 100) { set_error("jpeg_enable: quality must be in [1, 100]"); return EDGEHIP_ERR_ARG; }
    if (clen > 65533) { set_error("jpeg_enable: a COM segment holds at most 65533 bytes"); return EDGEHIP_ERR_ARG; }
    if (rebvo::jpeg::bound(c->plan.w, c->plan.h, clen) > 0x7FFFFFF0u) { set_error("jpeg_enable: the frame's worst-case stream does not fit in 31 bits"); return EDGEHIP_ERR_ARG; }
    const std::vector<uint8_t> hdr = rebvo::jpeg::header(c->plan.w, c->plan.h, quality, comment, clen);
    if (cap_bytes < hdr.size() + 2 || cap_bytes > 0x7FFFFFF0u) { set_error("jpeg_enable: cap_bytes is below header + EOI (or above 2 GiB)"); return EDGEHIP_ERR_ARG; }
    jpeg_free(c);
    auto *d = c->jpeg = new edgehip_ctx::JpegStore;
    const size_t B = c->plan.nseq;
    d->quality = quality;
    d->cap = cap_bytes;
    d->stride = ((size_t)cap_bytes + 15) & ~(size_t)15;
    d->hlen = (int)hdr.size();
    const size_t o_sizes = B * d->stride, o_tab = o_sizes + ((B * sizeof(edgehip_jpeg_size) + 15) & ~(size_t)15), o_hdr = o_tab + sizeof(JpegTables);
    const size_t o_fidx = o_hdr + ((hdr.size() + 15) & ~(size_t)15), o_mask = o_fidx + ((B * sizeof(int32_t) + 15) & ~(size_t)15), bytes = o_mask + B;
    if (hipMalloc(&d->arena, bytes) != hipSuccess || hipEventCreateWithFlags(&d->ev_done, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        jpeg_free(c);
        set_error("jpeg_enable: allocation failed");
        return EDGEHIP_ERR_MEMORY;
    }
    uint8_t *base = (uint8_t *)d->arena;
    d->out = base;
    d->sizes = (edgehip_jpeg_size *)(base + o_sizes);
    d->tab = (JpegTables *)(base + o_tab);
    d->hdr = base + o_hdr;
    d->fidx = (int32_t *)(base + o_fidx);
    d->mask = base + o_mask;
    JpegTables t;
    jpeg_tables(quality, &t);
    hipError_t e = hipMemsetAsync(d->arena, 0, bytes, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d->tab, &t, sizeof t, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d->hdr, hdr.data(), hdr.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // (t and hdr are free on return)
    if (e != hipSuccess) jpeg_free(c);
    EH_CHECK(e);
    return 0;
}

int edgehip_jpeg_select(edgehip_ctx *c, const uint8_t *mask) {
    EH_ENTER(c);
    auto *d = c->jpeg;
    if (!d) { set_error("jpeg_select: the JPEG store is not enabled (edgehip_jpeg_enable)"); return EDGEHIP_ERR_STATE; }
    if (!mask) { d->masked = false; return 0; }
    EH_CHECK(hipMemcpyAsync(d->mask, mask, c->plan.nseq, hipMemcpyHostToDevice, c->stream));
    EH_CHECK(hipStreamSynchronize(c->stream));   // (the caller's array is free on return)
    d->masked = true;
    return 0;
}

// the encoder on `slot` behind everything that writes the slot's frames; images = sequences (req == nullptr) or the sequences req[images] names
static int jpeg_launch(edgehip_ctx *c, const char *who, int slot, int images, const int32_t *req, uint8_t *out, edgehip_jpeg_size *sizes, bool masked) {
    auto *d = c->jpeg;
    if (!d) { set_error(std::string(who) + ": the JPEG store is not enabled (edgehip_jpeg_enable)"); return EDGEHIP_ERR_STATE; }
    if (slot < 0 || slot >= c->plan.nslots) { set_error(std::string(who) + ": slot out of range"); return EDGEHIP_ERR_ARG; }
    const edgehip_ctx::SlotSrc &ss = c->slot_src[slot];
    const size_t B = c->plan.nseq, n = c->plan.n;
    if (ss.grey8 && !ss.base && !c->grey8) { set_error(std::string(who) + ": the slot is marked 8-bit mono but the context has no 8-bit storage"); return EDGEHIP_ERR_STATE; }
    // the slot's frame is in place once the uploads into it have finished (stream_up, stream_a); the flag stays for stage A
    if (c->up_valid[slot]) EH_CHECK(hipStreamWaitEvent(c->stream, c->ev_up[slot], 0));
    if (int e = order_bc_after_a(c)) return e;
    JpegArgs a = {};
    // where stage A reads the slot's frames: its own storage (sequence-major) or frames of a bound pool, RGB24 or 8-bit mono
    if (ss.grey8) a.grey8 = ss.base ? ss.base : c->grey8 + (size_t)slot * B * n;
    else a.rgb = ss.base ? ss.base : rgbof(c, slot);
    if (ss.base) {   // the binding's indices in a row of the store's own: the page-locked row stage A reads is rewritten eight frames later
        EH_CHECK(hipMemcpyAsync(d->fidx, ss.host_idx.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice, c->stream));
        a.fidx = d->fidx;
    }
    a.und_base = c->und_base;
    a.und_iw = c->und_iw;
    a.tab = d->tab;
    a.hdr = d->hdr;
    a.out = out;
    a.sizes = sizes;
    a.mask = masked ? d->mask : nullptr;
    a.req = req;
    a.stride = d->stride;
    a.cap = d->cap;
    a.hlen = d->hlen;
    a.w = c->plan.w; a.h = c->plan.h; a.n = (int)n;
    hipLaunchKernelGGL(k_jpeg_encode, dim3((unsigned)images), dim3(kJpThreads), 0, c->stream, a);
    EH_LAUNCH_CHECK();
    // nothing else on this stream reads a slot's frame storage behind its stage A: whoever writes the slot next — an upload on either
    // upload stream — waits for the encoder's reads
    EH_CHECK(hipEventRecord(d->ev_done, c->stream));
    if (c->stream_a != c->stream) EH_CHECK(hipStreamWaitEvent(c->stream_a, d->ev_done, 0));
    EH_CHECK(hipStreamWaitEvent(c->stream_up, d->ev_done, 0));
    return 0;
}

int edgehip_jpeg_encode(edgehip_ctx *c, int slot) {
    EH_ENTER(c);
    auto *d = c->jpeg;
    return jpeg_launch(c, "jpeg_encode", slot, c->plan.nseq, nullptr, d ? d->out : nullptr, d ? d->sizes : nullptr, d && d->masked);
}

// ---- output callbacks at full pipeline depth, through c->jpeg_ring (export_ring.h) ----
// An entry: [n_cap] regions of the store's stride, then [n_cap] size records.  Its request row: [n_cap] sequence ids, then [n_cap] size
// records, which a copy on the ring's stream brings over right behind the encoder so that the fetch knows how many bytes to ask for.
int edgehip_jpeg_export(edgehip_ctx *c, int slot, int n, const int32_t *seqs, int *ticket_out) {
    EH_ENTER(c);
    auto *d = c->jpeg;
    if (!d) { set_error("jpeg_export: the JPEG store is not enabled (edgehip_jpeg_enable)"); return EDGEHIP_ERR_STATE; }
    if (n < 1 || !seqs || !ticket_out) { set_error("jpeg_export: bad argument"); return EDGEHIP_ERR_ARG; }
    if (slot < 0 || slot >= c->plan.nslots) { set_error("jpeg_export: slot out of range"); return EDGEHIP_ERR_ARG; }
    for (int j = 0; j < n; j++)
        if (seqs[j] < 0 || seqs[j] >= c->plan.nseq) { set_error("jpeg_export: sequence out of range"); return EDGEHIP_ERR_ARG; }
    ExportRing &x = c->jpeg_ring;
    if (int er = x.open(false)) return er;
    for (hipEvent_t &e : d->ev_sizes)
        if (!e) EH_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (n > x.n_cap) {
        if (int er = x.reserve(c, "jpeg_export", n, (d->stride + sizeof(edgehip_jpeg_size)) * n, (sizeof(int32_t) + sizeof(edgehip_jpeg_size)) * n + 8)) return er;
    }
    int e = 0;
    if (int er = x.claim("jpeg_export", &e)) return er;
    int32_t *req = (int32_t *)x.row(e);
    for (int j = 0; j < n; j++) req[j] = seqs[j];
    edgehip_jpeg_size *sizes_dev = (edgehip_jpeg_size *)(x.entry(e) + d->stride * x.n_cap);
    if (int er = jpeg_launch(c, "jpeg_export", slot, n, req, x.entry(e), sizes_dev, false)) return er;
    if (int er = x.commit(c, e, slot, n, 0, ticket_out)) return er;
    edgehip_jpeg_size *sizes_row = (edgehip_jpeg_size *)(x.row(e) + ((sizeof(int32_t) * x.n_cap + 7) & ~(size_t)7));
    EH_CHECK(hipStreamWaitEvent(x.stream, x.ev_pack[e], 0));
    EH_CHECK(hipMemcpyAsync(sizes_row, sizes_dev, sizeof(edgehip_jpeg_size) * n, hipMemcpyDeviceToHost, x.stream));
    EH_CHECK(hipEventRecord(d->ev_sizes[e], x.stream));
    return 0;
}

int edgehip_jpeg_export_sizes(edgehip_ctx *c, int ticket, edgehip_jpeg_size *sizes) {
    EH_ENTER(c);
    auto *d = c->jpeg;
    int e = 0;
    ExportRing &x = c->jpeg_ring;
    auto *t = d ? x.find(ticket, &e) : nullptr;
    if (!t || !sizes) { set_error("jpeg_export_sizes: unknown ticket or null argument"); return EDGEHIP_ERR_ARG; }
    EH_CHECK(hipEventSynchronize(d->ev_sizes[e]));   // the encoder of this ticket has run; nothing else is waited for
    memcpy(sizes, x.row(e) + ((sizeof(int32_t) * x.n_cap + 7) & ~(size_t)7), sizeof(edgehip_jpeg_size) * t->n);
    return 0;
}

int edgehip_jpeg_export_fetch(edgehip_ctx *c, int ticket, uint8_t *const *dst) {
    EH_ENTER(c);
    auto *d = c->jpeg;
    int e = 0;
    ExportRing &x = c->jpeg_ring;
    auto *t = d ? x.find(ticket, &e) : nullptr;
    if (!t || !dst) { set_error("jpeg_export_fetch: unknown ticket or null argument"); return EDGEHIP_ERR_ARG; }
    if (t->fetched) { set_error("jpeg_export_fetch: ticket already fetched"); return EDGEHIP_ERR_STATE; }
    EH_CHECK(hipEventSynchronize(d->ev_sizes[e]));
    const edgehip_jpeg_size *sz = (const edgehip_jpeg_size *)(x.row(e) + ((sizeof(int32_t) * x.n_cap + 7) & ~(size_t)7));
    std::vector<ExportRing::Copy> copies;
    for (int j = 0; j < t->n; j++) {
        const size_t nb = std::min(sz[j].size, d->cap);
        if (dst[j] && nb > 0) copies.push_back({dst[j], (size_t)j * d->stride, nb});   // (a null destination is skipped)
    }
    return x.fetch("jpeg_export_fetch", e, copies);
}

int edgehip_jpeg_export_wait(edgehip_ctx *c, int ticket) {
    EH_ENTER(c);
    int e = 0;
    if (!c->jpeg_ring.find(ticket, &e)) { set_error("jpeg_export_wait: unknown ticket"); return EDGEHIP_ERR_ARG; }
    return c->jpeg_ring.release(e);
}

int edgehip_download_jpeg_batch(edgehip_ctx *c, int n, const int32_t *seqs, uint8_t *const *dst, uint32_t cap, edgehip_jpeg_size *sizes) {
    EH_ENTER(c);
    auto *d = c->jpeg;
    if (!d) { set_error("download_jpeg: the JPEG store is not enabled"); return EDGEHIP_ERR_STATE; }
    if (n < 1 || !seqs) { set_error("download_jpeg: bad argument"); return EDGEHIP_ERR_ARG; }
    for (int j = 0; j < n; j++)
        if (seqs[j] < 0 || seqs[j] >= c->plan.nseq) { set_error("download_jpeg: sequence out of range"); return EDGEHIP_ERR_ARG; }
    // the size records first (one copy): they say how many bytes exist
    std::vector<edgehip_jpeg_size> s(c->plan.nseq);
    EH_CHECK(hipMemcpyAsync(s.data(), d->sizes, sizeof(edgehip_jpeg_size) * s.size(), hipMemcpyDeviceToHost, c->stream));
    EH_CHECK(hipStreamSynchronize(c->stream));
    bool any = false;
    for (int j = 0; j < n; j++) {
        if (sizes) sizes[j] = s[seqs[j]];
        const size_t nb = std::min<size_t>(std::min(s[seqs[j]].size, d->cap), cap);
        if (dst && dst[j] && nb > 0) {
            EH_CHECK(hipMemcpyAsync(dst[j], d->out + (size_t)seqs[j] * d->stride, nb, hipMemcpyDeviceToHost, c->stream));
            any = true;
        }
    }
    if (any) EH_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int edgehip_download_jpeg(edgehip_ctx *c, int seq, uint8_t *dst, uint32_t cap, edgehip_jpeg_size *size) {
    return edgehip_download_jpeg_batch(c, 1, &seq, &dst, cap, size);
}

int edgehip_jpeg_device(edgehip_ctx *c, int first, int count, void *bytes_dev, void *sizes_dev) {
    EH_ENTER(c);
    auto *d = c->jpeg;
    if (!d) { set_error("jpeg_device: the JPEG store is not enabled"); return EDGEHIP_ERR_STATE; }
    if (first < 0 || count < 1 || first + count > c->plan.nseq) { set_error("jpeg_device: sequence range out of bounds"); return EDGEHIP_ERR_ARG; }
    if (bytes_dev) EH_CHECK(hipMemcpyAsync(bytes_dev, d->out + first * d->stride, d->stride * count, hipMemcpyDeviceToDevice, c->stream));
    if (sizes_dev) EH_CHECK(hipMemcpyAsync(sizes_dev, d->sizes + first, sizeof(edgehip_jpeg_size) * count, hipMemcpyDeviceToDevice, c->stream));
    EH_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int edgehip_jpeg_encode_images(edgehip_ctx *c, const void *rgb24_dev, int w, int h, int count, int quality, void *out_dev, uint32_t cap,
                               void *sizes_dev) {
    EH_ENTER(c);
    if (!rgb24_dev || !out_dev || !sizes_dev || w < 1 || h < 1 || w > 65535 || h > 65535 || count < 1 || (size_t)w * h > 0x7FFFFFFFu / 3) {
        set_error("jpeg_encode_images: bad argument (images of 1x1 .. 65535x65535 with w * h * 3 < 2^31, count >= 1)");
        return EDGEHIP_ERR_ARG;
    }
    if (rebvo::jpeg::bound(w, h, 0) > 0x7FFFFFF0u) { set_error("jpeg_encode_images: the image's worst-case stream (edgehip_jpeg_bound) does not fit in 31 bits"); return EDGEHIP_ERR_ARG; }
    if (quality < 1 || quality > 100) { set_error("jpeg_encode_images: quality must be in [1, 100]"); return EDGEHIP_ERR_ARG; }
    if (cap < rebvo::jpeg::kHeaderBytes + 2 || (cap & 15) || ((uintptr_t)out_dev & 15) || cap > 0x7FFFFFF0u) {
        set_error("jpeg_encode_images: cap must be a multiple of 16, at least header + EOI, and out_dev 16-byte aligned");
        return EDGEHIP_ERR_ARG;
    }
    // a stage-level entry: tables and header of this call live in scratch of its own, and the call returns when the images are done
    const std::vector<uint8_t> hdr = rebvo::jpeg::header(w, h, quality, nullptr, 0);
    JpegTables t;
    jpeg_tables(quality, &t);
    void *scratch = nullptr;
    if (hipMalloc(&scratch, sizeof t + ((hdr.size() + 15) & ~(size_t)15)) != hipSuccess) {
        (void)hipGetLastError();
        set_error("jpeg_encode_images: allocation failed");
        return EDGEHIP_ERR_MEMORY;
    }
    JpegArgs a = {};
    a.rgb = (const uint8_t *)rgb24_dev;
    a.tab = (JpegTables *)scratch;
    a.hdr = (uint8_t *)scratch + sizeof t;
    a.out = (uint8_t *)out_dev;
    a.sizes = (edgehip_jpeg_size *)sizes_dev;
    a.stride = cap;
    a.cap = cap;
    a.hlen = (int)hdr.size();
    a.w = w; a.h = h; a.n = w * h;
    hipError_t e = hipMemcpyAsync(scratch, &t, sizeof t, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync((uint8_t *)scratch + sizeof t, hdr.data(), hdr.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_jpeg_encode, dim3((unsigned)count), dim3(kJpThreads), 0, c->stream, a);
        e = hipGetLastError();
    }
    const hipError_t e2 = hipStreamSynchronize(c->stream);
    (void)hipFree(scratch);
    EH_CHECK(e);
    EH_CHECK(e2);
    return 0;
}
