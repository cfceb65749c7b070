// jpeg_decode.hip — baseline JPEG camera frames decoded on the device (MJPEG ingest): the counterpart of jpeg_encode.hip.  The rule is the
// host reader's (rebvo_amd/host/src/jpeg_reader.cpp), i.e. libjpeg's at its defaults: Huffman decoding, jpeg_idct_islow, fancy upsampling,
// ycc_rgb_convert, all in integers.  The host parses the markers (rebvo/jpeg_decode.h) and cuts the scan into groups of whole restart
// intervals (jpeg_entropy.h: plan_chains); the entropy-coded bytes and one descriptor per stream go up, and three launches follow:
//   k_jpeg_entropy  one wave per (stream, group).  Every lane runs the chain walk of jpeg_entropy.h on the same values; what is order-free
//                   is spread over the lanes: the stream is staged through a 1 KB window in LDS, 16 bytes per lane, and lane k keeps
//                   coefficient k of the current block, so a finished block leaves as one 128-byte store.  Tables live in LDS.
//   k_jpeg_idct     dequantisation and jpeg_idct_islow: a thread per block column, then per block row, into one 8-bit sample plane per
//                   component (whole MCUs, 1 B per padded sample).
//   k_jpeg_pixels   upsampling with libjpeg's edge rules and the colour conversion, a thread per pixel, into an LDS image of the
//                   workgroup's output bytes that leaves through flush_words' 16-byte stores (pack_flush.h).  Padding is never written.
// The upsampling reads chroma samples of neighbouring blocks, which is why the samples pass through memory between the last two.
// A stream's coefficients, samples and pixels depend on its own bytes and descriptor only.
#include "ctx.h"
#include "pack_flush.h"
#include "jpeg_entropy.h"
#include "jpeg_pixels.h"

#include <algorithm>
#include <vector>

namespace edgehip {
namespace jd = rebvo::jpegdec;

struct DevStream {
    jd::Stream d;
    jd::ChainPlan p;
    uint64_t bytes_off;   // the stream's entropy-coded segment inside the call's byte region (a multiple of 16)
};
static_assert(sizeof(DevStream) % 16 == 0 && sizeof(jd::Stream) % 4 == 0, "copied in words");

constexpr int kJdWindow = 1024;      // bytes of the stream in LDS: 64 lanes x 16
constexpr int kJdIdctBlocks = 32;    // blocks per workgroup of k_jpeg_idct (256 threads: 8 per block)
constexpr int kJdPixels = 1024;      // pixels per workgroup of k_jpeg_pixels

struct WaveSrc {   // the segment through a window in LDS; every lane asks for the same position
    const uint8_t *g;   // 16-byte aligned; whole 16-byte words up to len rounded up are readable
    uint32_t len, base;
    uint8_t *win;
    __device__ void refill(uint32_t pos) {
        typedef uint32_t u4v __attribute__((ext_vector_type(4)));
        base = pos & ~15u;
        __syncthreads();   // (one wave per workgroup: orders the lanes' LDS reads before the overwrite)
        const uint32_t o = base + threadIdx.x * 16;
        u4v v = {0u, 0u, 0u, 0u};
        if (o < len) v = *reinterpret_cast<const u4v *>(g + o);
        reinterpret_cast<u4v *>(win)[threadIdx.x] = v;
        __syncthreads();
    }
    __device__ int byte(uint32_t pos) {
        if (pos - base >= (uint32_t)kJdWindow) refill(pos);
        return win[pos - base];
    }
};
struct LaneSink {   // lane k holds coefficient k (natural order) of the block being decoded
    int16_t *coef;
    int v;
    __device__ void begin_block() { v = 0; }
    __device__ void put(int k, int val) { if ((int)threadIdx.x == k) v = val; }
    __device__ void note(int, int) {}
    __device__ void end_block(int block) { coef[(size_t)block * 64 + threadIdx.x] = (int16_t)v; }
};

__global__ __launch_bounds__(64) void k_jpeg_entropy(const DevStream *__restrict__ ds, const uint8_t *__restrict__ bytes, int16_t *__restrict__ coef,
                                                      size_t blocks_stride, int32_t *__restrict__ status) {
    __shared__ __attribute__((aligned(16))) jd::Stream s;
    __shared__ __attribute__((aligned(16))) uint8_t win[kJdWindow];
    const DevStream &S = ds[blockIdx.y];
    const int g = blockIdx.x;
    if (g >= S.p.ngroups) return;
    for (int i = threadIdx.x; i < (int)(sizeof(jd::Stream) / 4); i += 64)
        reinterpret_cast<uint32_t *>(&s)[i] = reinterpret_cast<const uint32_t *>(&S.d)[i];
    __syncthreads();
    const int nmcu = s.mcux * s.mcuy, first = g * S.p.group_mcus;
    const int count = min(S.p.group_mcus, nmcu - first);
    if (count <= 0) return;
    WaveSrc src = {bytes + S.bytes_off, s.ecs_len, 0u, win};
    src.refill(min(S.p.off[g], s.ecs_len));
    LaneSink sink = {coef + (size_t)blockIdx.y * blocks_stride * 64, 0};
    const int st = jd::chain_walk(s, first, count, S.p.off[g], s.ecs_len, src, sink, nullptr);
    if (st && threadIdx.x == 0) atomicMax(&status[blockIdx.y], st);
}

__global__ __launch_bounds__(256) void k_jpeg_idct(const DevStream *__restrict__ ds, const int16_t *__restrict__ coef, uint8_t *__restrict__ samples,
                                                    size_t blocks_stride) {
    __shared__ int ws[kJdIdctBlocks][65];
    const jd::Stream &s = ds[blockIdx.y].d;
    const int nblocks = s.nblocks;
    const int blk = blockIdx.x * kJdIdctBlocks + (threadIdx.x >> 3), lane8 = threadIdx.x & 7;
    const bool live = blk < nblocks;
    int ci = 0;
    if (live) ci = (s.ncomp == 3 && blk >= s.comp[1].block_base) ? (blk >= s.comp[2].block_base ? 2 : 1) : 0;
    if (live) {   // pass 1: column lane8 of the block
        const int16_t *cf = coef + ((size_t)blockIdx.y * blocks_stride + blk) * 64;
        const uint16_t *q = s.q[s.comp[ci].tq];
        int in[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; r++) in[r] = (int)cf[8 * r + lane8] * (int)q[8 * r + lane8];
        jd::px_idct_col(in, o);
#pragma unroll
        for (int r = 0; r < 8; r++) ws[threadIdx.x >> 3][8 * r + lane8] = o[r];
    }
    __syncthreads();
    if (live) {   // pass 2: row lane8 of the block
        const jd::Comp &c = s.comp[ci];
        const int local = blk - c.block_base, brow = local / c.wblocks, bcol = local - brow * c.wblocks;
        int w8[8];
#pragma unroll
        for (int k = 0; k < 8; k++) w8[k] = ws[threadIdx.x >> 3][8 * lane8 + k];
        uint8_t px[8];
        jd::px_idct_row(w8, px);
        uint8_t *dst = samples + ((size_t)blockIdx.y * blocks_stride + c.block_base) * 64 + (size_t)(brow * 8 + lane8) * (c.wblocks * 8) + (size_t)bcol * 8;
        uint2 v;
        v.x = (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16) | ((uint32_t)px[3] << 24);
        v.y = (uint32_t)px[4] | ((uint32_t)px[5] << 8) | ((uint32_t)px[6] << 16) | ((uint32_t)px[7] << 24);
        *reinterpret_cast<uint2 *>(dst) = v;   // (8-byte aligned: every term is a multiple of 8)
    }
}

// out: stream j's frame at out + j * npix * bpp (bpp 3: RGB24, 1: the 8-bit plane of a one-component stream); out need not be aligned
__global__ __launch_bounds__(256) void k_jpeg_pixels(const DevStream *__restrict__ ds, const uint8_t *__restrict__ samples, size_t blocks_stride,
                                                      uint8_t *out, int bpp) {
    __shared__ __attribute__((aligned(16))) uint8_t img[kJdPixels * 3 + 32];
    const jd::Stream &s = ds[blockIdx.y].d;
    const int npix = s.w * s.h, p0 = blockIdx.x * kJdPixels;
    if (p0 >= npix) return;
    const int cnt = min(kJdPixels, npix - p0);
    uint8_t *store = reinterpret_cast<uint8_t *>(reinterpret_cast<uintptr_t>(out) & ~(uintptr_t)15);
    const size_t b0 = (size_t)(out - store) + ((size_t)blockIdx.y * npix + p0) * bpp, b1 = b0 + (size_t)cnt * bpp, w0 = b0 & ~(size_t)15;
    const uint8_t *sp = samples + (size_t)blockIdx.y * blocks_stride * 64;
    for (int i = threadIdx.x; i < cnt; i += 256) {
        const int p = p0 + i, y = p / s.w, x = p - y * s.w;
        const uint32_t v = jd::px_pixel(s, sp, x, y);
        uint8_t *o = img + (b0 - w0) + (size_t)i * bpp;
        o[0] = (uint8_t)v;
        if (bpp == 3) { o[1] = (uint8_t)(v >> 8); o[2] = (uint8_t)(v >> 16); }
    }
    __syncthreads();
    flush_words<uint8_t, 256>(img, store, w0, (int)((b1 - w0 + 15) / 16), b0, b1);
}

}  // namespace edgehip

using namespace edgehip;

struct edgehip_ctx::JpegDec {
    int max_streams = 0;
    uint32_t cap = 0;
    size_t stride = 0;        // bytes of one stream's region: cap rounded up to 16
    size_t blocks = 0;        // blocks per stream in the coefficient and sample planes: any sampling of the context's w x h fits
    uint8_t *pin_bytes = nullptr, *dev_bytes = nullptr;
    DevStream *pin_desc = nullptr, *dev_desc = nullptr;
    int16_t *coef = nullptr;
    uint8_t *samples = nullptr;
    int32_t *status = nullptr;   // [nslots][nseq] the walk's status per sequence of each slot's last compressed upload
    hipEvent_t ev_copied = nullptr;   // the last copies out of the page-locked regions have finished
    bool busy = false;
    hipEvent_t ev_t[4] = {nullptr, nullptr, nullptr, nullptr};   // around the three kernels of an upload made under edgehip_profile_enable
    bool timed = false;          // the last upload recorded them
    uint64_t moved = 0;          // bytes of the last upload's two copies (segments, descriptors)
};

void edgehip::jpeg_decode_free(edgehip_ctx *c) {
    auto *d = c->jpegdec;
    if (!d) return;
    (void)hipStreamSynchronize(c->stream_up);
    if (d->pin_bytes) (void)hipHostFree(d->pin_bytes);
    if (d->pin_desc) (void)hipHostFree(d->pin_desc);
    for (void *p : {(void *)d->dev_bytes, (void *)d->dev_desc, (void *)d->coef, (void *)d->samples, (void *)d->status})
        if (p) (void)hipFree(p);
    if (d->ev_copied) (void)hipEventDestroy(d->ev_copied);
    for (hipEvent_t e : d->ev_t) if (e) (void)hipEventDestroy(e);
    delete d;
    c->jpegdec = nullptr;
}

static void fill_info(const jd::Stream &s, edgehip_jpeg_info *info) {
    const jd::Info i = jd::info_of(s);
    static_assert(sizeof(jd::Info) == sizeof(edgehip_jpeg_info), "one layout");
    memcpy(info, &i, sizeof i);
}

int edgehip_jpeg_probe(const uint8_t *data, size_t len, edgehip_jpeg_info *info) {
    if (!info) { set_error("jpeg_probe: null argument"); return EDGEHIP_ERR_ARG; }
    jd::Stream s;
    jd::parse(data, len, s);
    fill_info(s, info);
    return 0;
}

// the three launches over `count` streams whose descriptors and bytes are (or will be, in stream order) on the device
static int decode_enqueue(hipStream_t st, const DevStream *host_desc, int count, const DevStream *dev_desc, const uint8_t *dev_bytes, int16_t *coef,
                          uint8_t *samples, size_t blocks, int32_t *status, uint8_t *out, int bpp, hipEvent_t *ev_t = nullptr /* [4] or null */) {
    int groups = 1, nblocks = 1, npix = 1;
    for (int j = 0; j < count; j++) {
        groups = std::max(groups, host_desc[j].p.ngroups);
        nblocks = std::max(nblocks, host_desc[j].d.nblocks);
        npix = std::max(npix, host_desc[j].d.w * host_desc[j].d.h);
    }
    EH_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t) * count, st));
    if (ev_t) EH_CHECK(hipEventRecord(ev_t[0], st));
    hipLaunchKernelGGL(k_jpeg_entropy, dim3((unsigned)groups, (unsigned)count), dim3(64), 0, st, dev_desc, dev_bytes, coef, blocks, status);
    EH_LAUNCH_CHECK();
    if (ev_t) EH_CHECK(hipEventRecord(ev_t[1], st));
    hipLaunchKernelGGL(k_jpeg_idct, dim3((unsigned)((nblocks + kJdIdctBlocks - 1) / kJdIdctBlocks), (unsigned)count), dim3(256), 0, st, dev_desc, coef,
                       samples, blocks);
    EH_LAUNCH_CHECK();
    if (ev_t) EH_CHECK(hipEventRecord(ev_t[2], st));
    hipLaunchKernelGGL(k_jpeg_pixels, dim3((unsigned)((npix + kJdPixels - 1) / kJdPixels), (unsigned)count), dim3(256), 0, st, dev_desc, samples, blocks,
                       out, bpp);
    EH_LAUNCH_CHECK();
    if (ev_t) EH_CHECK(hipEventRecord(ev_t[3], st));
    return 0;
}

int edgehip_jpeg_decode_enable(edgehip_ctx *c, int max_streams, uint32_t cap_bytes) {
    EH_ENTER(c);
    if (cap_bytes == 0) { jpeg_decode_free(c); return 0; }
    if (max_streams < 1 || max_streams > c->plan.nseq || cap_bytes > 0x7FFFFFF0u) {
        set_error("jpeg_decode_enable: max_streams must be in [1, nseq] and cap_bytes below 2 GiB");
        return EDGEHIP_ERR_ARG;
    }
    jpeg_decode_free(c);
    auto *d = c->jpegdec = new edgehip_ctx::JpegDec;
    d->max_streams = max_streams;
    d->cap = cap_bytes;
    d->stride = ((size_t)cap_bytes + 15) & ~(size_t)15;
    d->blocks = (size_t)12 * ((c->plan.w + 15) / 16) * ((c->plan.h + 15) / 16);
    const size_t M = max_streams, nstat = (size_t)c->plan.nslots * c->plan.nseq;
    bool ok = hipHostMalloc((void **)&d->pin_bytes, M * d->stride, hipHostMallocDefault) == hipSuccess &&
              hipHostMalloc((void **)&d->pin_desc, M * sizeof(DevStream), hipHostMallocDefault) == hipSuccess &&
              hipMalloc((void **)&d->dev_bytes, M * d->stride) == hipSuccess && hipMalloc((void **)&d->dev_desc, M * sizeof(DevStream)) == hipSuccess &&
              hipMalloc((void **)&d->coef, M * d->blocks * 128) == hipSuccess && hipMalloc((void **)&d->samples, M * d->blocks * 64) == hipSuccess &&
              hipMalloc((void **)&d->status, nstat * sizeof(int32_t)) == hipSuccess &&
              hipEventCreateWithFlags(&d->ev_copied, hipEventDisableTiming) == hipSuccess;
    for (hipEvent_t &e : d->ev_t) ok = ok && hipEventCreate(&e) == hipSuccess;
    if (ok) ok = hipMemsetAsync(d->status, 0, nstat * sizeof(int32_t), c->stream_up) == hipSuccess && hipStreamSynchronize(c->stream_up) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        jpeg_decode_free(c);
        set_error("jpeg_decode_enable: allocation failed");
        return EDGEHIP_ERR_MEMORY;
    }
    return 0;
}

int edgehip_upload_jpeg(edgehip_ctx *c, int slot, const uint8_t *const *data, const size_t *len, int seq_first, int count, int format, int32_t *reason_out) {
    EH_ENTER(c);
    auto *d = c->jpegdec;
    if (!d) { set_error("upload_jpeg: the decoder is not enabled (edgehip_jpeg_decode_enable)"); return EDGEHIP_ERR_STATE; }
    if (slot < 0 || slot >= c->plan.nslots) { set_error("upload_jpeg: slot out of range"); return EDGEHIP_ERR_ARG; }
    if (!data || !len || seq_first < 0 || count < 1 || seq_first + count > c->plan.nseq || count > d->max_streams ||
        (format != EDGEHIP_FRAME_RGB24 && format != EDGEHIP_FRAME_GREY8)) {
        set_error("upload_jpeg: bad range, more streams than max_streams, or an unknown format");
        return EDGEHIP_ERR_ARG;
    }
    // headers first, into memory of the call's own: nothing changes unless every stream is decodable
    std::vector<DevStream> desc(count);
    bool refuse = false, colour = false;
    size_t total = 0;
    for (int j = 0; j < count; j++) {
        jd::Stream &s = desc[j].d;
        jd::parse(data[j], data[j] ? len[j] : 0, s);
        jd::expect(s, c->plan.w, c->plan.h, d->cap);
        if (reason_out) reason_out[j] = s.reason;
        refuse |= s.reason != 0;
        colour |= s.ncomp != 1;
        desc[j].bytes_off = total;
        total += ((size_t)s.ecs_len + 15) & ~(size_t)15;
    }
    if (refuse) { set_error("upload_jpeg: a stream is not decodable on the device (reason_out); nothing was enqueued"); return EDGEHIP_ERR_ARG; }
    const bool grey8 = format == EDGEHIP_FRAME_GREY8;
    if (grey8 && colour) { set_error("upload_jpeg: a colour stream cannot go into an 8-bit mono slot"); return EDGEHIP_ERR_ARG; }
    if (grey8)
        if (int e = ensure_grey8(c)) return e;
    if (d->busy) EH_CHECK(hipEventSynchronize(d->ev_copied));   // the page-locked regions are reused
    for (int j = 0; j < count; j++) {
        const jd::Stream &s = desc[j].d;
        jd::plan_chains(data[j] + s.ecs_off, s, desc[j].p);
        memcpy(d->pin_bytes + desc[j].bytes_off, data[j] + s.ecs_off, s.ecs_len);
        d->pin_desc[j] = desc[j];
    }
    unbind_rgb(c, slot, grey8);
    if (int e = upload_waits_for_slot(c, slot)) return e;
    EH_CHECK(hipMemcpyAsync(d->dev_bytes, d->pin_bytes, total, hipMemcpyHostToDevice, c->stream_up));
    EH_CHECK(hipMemcpyAsync(d->dev_desc, d->pin_desc, sizeof(DevStream) * count, hipMemcpyHostToDevice, c->stream_up));
    EH_CHECK(hipEventRecord(d->ev_copied, c->stream_up));
    d->busy = true;
    const size_t n = c->plan.n;
    uint8_t *out = grey8 ? c->grey8 + ((size_t)slot * c->plan.nseq + seq_first) * n : rgbof(c, slot) + (size_t)seq_first * n * 3;
    if (int e = decode_enqueue(c->stream_up, desc.data(), count, d->dev_desc, d->dev_bytes, d->coef, d->samples, d->blocks,
                               d->status + (size_t)slot * c->plan.nseq + seq_first, out, grey8 ? 1 : 3, c->prof->on ? d->ev_t : nullptr)) return e;
    d->timed = c->prof->on;
    d->moved = total + sizeof(DevStream) * count;
    EH_CHECK(hipEventRecord(c->ev_up[slot], c->stream_up));
    c->up_valid[slot] = true;
    return 0;
}

int edgehip_read_jpeg_decode_status(edgehip_ctx *c, int slot, int32_t *status) {
    EH_ENTER(c);
    auto *d = c->jpegdec;
    if (!d) { set_error("read_jpeg_decode_status: the decoder is not enabled"); return EDGEHIP_ERR_STATE; }
    if (slot < 0 || slot >= c->plan.nslots || !status) { set_error("read_jpeg_decode_status: slot out of range or null argument"); return EDGEHIP_ERR_ARG; }
    EH_CHECK(hipMemcpyAsync(status, d->status + (size_t)slot * c->plan.nseq, sizeof(int32_t) * c->plan.nseq, hipMemcpyDeviceToHost, c->stream_up));
    EH_CHECK(hipStreamSynchronize(c->stream_up));
    return 0;
}

int edgehip_jpeg_decode_ms(edgehip_ctx *c, float *ms, uint64_t *bytes_moved) {
    EH_ENTER(c);
    auto *d = c->jpegdec;
    if (!d || !d->timed) { set_error("jpeg_decode_ms: the last compressed upload was not made under edgehip_profile_enable"); return EDGEHIP_ERR_STATE; }
    if (!ms) { set_error("jpeg_decode_ms: null argument"); return EDGEHIP_ERR_ARG; }
    if (bytes_moved) *bytes_moved = d->moved;
    EH_CHECK(hipEventSynchronize(d->ev_t[3]));
    for (int i = 0; i < 3; i++) EH_CHECK(hipEventElapsedTime(&ms[i], d->ev_t[i], d->ev_t[i + 1]));
    return 0;
}

int edgehip_jpeg_decode_images(edgehip_ctx *c, const uint8_t *const *data, const size_t *len, int count, int w, int h, void *rgb24_dev_out,
                               int32_t *reason_out) {
    EH_ENTER(c);
    if (!data || !len || !rgb24_dev_out || count < 1 || w < 1 || h < 1 || w > 16384 || h > 16384 || (size_t)w * h * 3 * count > 0x7FFFFFFFu) {
        set_error("jpeg_decode_images: bad argument (count >= 1, images of 1x1 .. 16384x16384, count * w * h * 3 < 2^31)");
        return EDGEHIP_ERR_ARG;
    }
    std::vector<DevStream> desc(count);
    bool refuse = false;
    size_t total = 0, blocks = 1;
    for (int j = 0; j < count; j++) {
        jd::Stream &s = desc[j].d;
        jd::parse(data[j], data[j] ? len[j] : 0, s);
        jd::expect(s, w, h, 0);
        if (reason_out) reason_out[j] = s.reason;
        refuse |= s.reason != 0;
        if (s.reason) continue;
        jd::plan_chains(data[j] + s.ecs_off, s, desc[j].p);
        desc[j].bytes_off = total;
        total += ((size_t)s.ecs_len + 15) & ~(size_t)15;
        blocks = std::max(blocks, (size_t)s.nblocks);
    }
    if (refuse) { set_error("jpeg_decode_images: a stream is not decodable on the device (reason_out)"); return EDGEHIP_ERR_ARG; }
    // a stage-level entry: everything lives in scratch of the call's own, and the call returns when the images are done
    std::vector<uint8_t> bytes(total + 16, 0);
    for (int j = 0; j < count; j++) memcpy(bytes.data() + desc[j].bytes_off, data[j] + desc[j].d.ecs_off, desc[j].d.ecs_len);
    const size_t o_bytes = sizeof(DevStream) * count, o_coef = o_bytes + ((bytes.size() + 15) & ~(size_t)15), o_samp = o_coef + blocks * 128 * count,
                 o_stat = o_samp + blocks * 64 * count;
    uint8_t *scratch = nullptr;
    if (hipMalloc((void **)&scratch, o_stat + sizeof(int32_t) * count) != hipSuccess) {
        (void)hipGetLastError();
        set_error("jpeg_decode_images: allocation failed");
        return EDGEHIP_ERR_MEMORY;
    }
    std::vector<int32_t> st(count, 0);
    hipError_t e = hipMemcpyAsync(scratch, desc.data(), sizeof(DevStream) * count, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(scratch + o_bytes, bytes.data(), bytes.size(), hipMemcpyHostToDevice, c->stream);
    int rc = 0;
    if (e == hipSuccess)
        rc = decode_enqueue(c->stream, desc.data(), count, (const DevStream *)scratch, scratch + o_bytes, (int16_t *)(scratch + o_coef), scratch + o_samp, blocks,
                            (int32_t *)(scratch + o_stat), (uint8_t *)rgb24_dev_out, 3);
    if (e == hipSuccess && rc == 0) e = hipMemcpyAsync(st.data(), scratch + o_stat, sizeof(int32_t) * count, hipMemcpyDeviceToHost, c->stream);
    const hipError_t e2 = hipStreamSynchronize(c->stream);
    (void)hipFree(scratch);
    if (rc) return rc;
    EH_CHECK(e);
    EH_CHECK(e2);
    bool corrupt = false;
    for (int j = 0; j < count; j++)
        if (st[j]) { corrupt = true; if (reason_out) reason_out[j] = EDGEHIP_JPEG_REASON_WALK + st[j]; }
    if (corrupt) { set_error("jpeg_decode_images: a stream's entropy-coded data is corrupt or short (reason_out)"); return EDGEHIP_ERR_ARG; }
    return 0;
}

int edgehip_download_frame(edgehip_ctx *c, int seq, int slot, uint8_t *out, int *format) {
    EH_ENTER(c);
    if (seq < 0 || seq >= c->plan.nseq || slot < 0 || slot >= c->plan.nslots || !out) { set_error("download_frame: sequence or slot out of range, or null"); return EDGEHIP_ERR_ARG; }
    const edgehip_ctx::SlotSrc &ss = c->slot_src[slot];
    if (ss.base) { set_error("download_frame: the slot reads a bound pool, not its own storage"); return EDGEHIP_ERR_STATE; }
    if (ss.grey8 && !c->grey8) { set_error("download_frame: the slot is marked 8-bit mono but the context has no 8-bit storage"); return EDGEHIP_ERR_STATE; }
    if (int e = sync_all(c)) return e;
    EH_CHECK(hipStreamSynchronize(c->stream_up));
    const size_t n = c->plan.n;
    const uint8_t *src = ss.grey8 ? c->grey8 + ((size_t)slot * c->plan.nseq + seq) * n : rgbof(c, slot) + (size_t)seq * n * 3;
    EH_CHECK(hipMemcpy(out, src, ss.grey8 ? n : n * 3, hipMemcpyDeviceToHost));
    if (format) *format = ss.grey8 ? EDGEHIP_FRAME_GREY8 : EDGEHIP_FRAME_RGB24;
    return 0;
}
