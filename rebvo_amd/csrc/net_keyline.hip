// net_keyline.hip — the reference's wire-format edge map (net_keyline, include/CommLib/net_keypoint.h:35-62) packed on the device:
// copy_net_keyline followed by copy_net_keyline_nextid (src/CommLib/net_keypoint.cpp:29-108), which its third thread runs per frame
// (src/rebvo/rebvo_third_t.cpp:189-203), for every sequence of a slot in one launch.
//
// Both passes collapse into one order-free rule per KeyLine: KeyLine j is packed iff j < count = min(kn, kl_size), into record j (the
// value the reference puts in net_id), and n_kl = n_id when 0 <= n_id < count, else -1.  Every field is formed by the reference's
// own operations: the float / double mix as written there, clamp_ushort / clamp_uchar on a float (include/UtilLib/util.h:52-66).
//
// The hot part is the store.  Records are 15 bytes and a sequence's records start at seq * kl_size * 15: aligned to nothing.  The
// output is therefore cut by ADDRESS, not by record: a workgroup owns kNkWords consecutive 16-byte words of the store, computes every
// record that touches them (16 records = 15 words; up to one record at either end is shared with the neighbour workgroup, which
// computes it too) into LDS at the byte position it has in those words, and flush_words (pack_flush.h) writes them out.  Only the
// first and the last word of a sequence's count * 15 bytes can be partial.  The SoA reads are coalesced (KeyLine j by lane j).
#include "ctx.h"
#include "pack_flush.h"

#include <cmath>
#include <vector>

namespace edgehip {

constexpr int kNkThreads = 256;
constexpr int kNkWords = 240;               // 16-byte words per workgroup: 3840 B = 256 records
constexpr int kNkBytes = kNkWords * 16;
constexpr double kNetRhoScaling = 10000.0;  // NET_RHO_SCALING, net_keypoint.h:32

struct NkArgs {
    const KlSoA *kls;            // [nseq] KeyLines of the slot
    const KlSoA *kls_pair;       // [nseq] KeyLines of the pair slot, or null
    const int32_t *kns;          // [nseq]
    const double *k_prof;        // [nseq] or null: SeqDev::pub.K
    const SeqDev *seqs;          // [nseq]
    uint8_t *rec;                // [nseq][kl_size][15]
    edgehip_net_header *hdr;     // [nseq]
    int kl_size, cap;
};

// util::clamp_uchar / clamp_ushort (include/UtilLib/util.h:52-66): the argument arrives as float
__device__ __forceinline__ uint32_t nk_clamp_uchar(float f) { return f < 0 ? 0u : f > 255.0f ? 255u : (uint32_t)(int)f; }
__device__ __forceinline__ uint32_t nk_clamp_ushort(float f) { return f < 0 ? 0u : f > 65535.0f ? 65535u : (uint32_t)(int)f; }
// (u_short) of round(float) as an x86-64 build converts it: cvttsd2si to 32 bits, low 16 bits kept
__device__ __forceinline__ uint32_t nk_round_u16(float v) { return (uint32_t)x86_cvttsd2si(round((double)v)) & 0xFFFFu; }
// to[j].rho = std::max(util::clamp_ushort(NET_RHO_SCALING * kl.rho / k_prof), (u_short)1): product and quotient in double, narrowed to float
__device__ __forceinline__ uint32_t nk_rho(double v, double k_prof) {
    const float f = (float)(kNetRhoScaling * v / k_prof);
    return max(nk_clamp_ushort(f), 1u);
}

__global__ __launch_bounds__(kNkThreads) void k_net_pack(NkArgs a) {
    __shared__ __align__(16) uint8_t buf[16 + kNkBytes + 16];   // the workgroup's words at buf + 16; a shared record may start up to 14 B before them
    const int seq = blockIdx.y, tid = threadIdx.x;
    const int count = max(0, min(min(a.kns[seq], a.kl_size), a.cap));
    double k_prof = 0;
    if (blockIdx.x == 0 || count > 0) k_prof = a.k_prof ? a.k_prof[seq] : a.seqs[seq].pub.K;
    if (blockIdx.x == 0 && tid == 0) {
        edgehip_net_header h;
        h.kline_num = count;
        h.km_num = a.seqs[seq].pub.klm_num;
        h.k = (float)k_prof;
        a.hdr[seq] = h;
    }
    // the sequence's bytes [lo, hi) of the store, and this workgroup's words [w0, w1) of them
    const size_t lo = (size_t)seq * a.kl_size * 15, hi = lo + (size_t)count * 15;
    const size_t w0 = (lo & ~(size_t)15) + (size_t)blockIdx.x * kNkBytes, w1 = w0 + kNkBytes;
    if (w0 >= hi) return;
    const size_t b0 = max(w0, lo), b1 = min(w1, hi);      // the bytes this workgroup writes
    const int r0 = (int)((b0 - lo) / 15), r1 = (int)((b1 - lo + 14) / 15);   // the records that touch them: at most 257

    const KlSoA &k = a.kls[seq];
    for (int j = r0 + tid; j < r1; j += kNkThreads) {
        const float2 cp = ldg(k.c_p, j);
        const uint32_t qx = nk_round_u16(cp.x), qy = nk_round_u16(cp.y);
        const uint32_t rho = nk_rho(ldg(k.rho, j), k_prof), s_rho = nk_rho(ldg(k.s_rho, j), k_prof);
        uint32_t fx = 127, fy = 127;
        if (a.kls_pair) {   // the stereo disparity (net_keypoint.cpp:45-58)
            const int sm = ldg(k.stereo_m_id, j);
            if (sm >= 0 && sm < a.cap) {
                const float2 pp = ldg(a.kls_pair[seq].c_p, sm);
                const float dx = -cp.x + pp.x, dy = -cp.y + pp.y;
                if (fabs(round((double)dx)) < 127 && fabs(round((double)dy)) < 127) {
                    fx = nk_clamp_uchar((float)round((double)dx + 127.0));
                    fy = nk_clamp_uchar((float)round((double)dy + 127.0));
                }
            }
        } else {            // the matched displacement (:60-61): subtraction and * 10 in float, + 127.0 in double
            const float2 pm = ldg(k.p_m, j), pm0 = ldg(k.p_m_0, j);
            const float dx = (pm.x - pm0.x) * 10, dy = (pm.y - pm0.y) * 10;
            fx = nk_clamp_uchar((float)round((double)dx + 127.0));
            fy = nk_clamp_uchar((float)round((double)dy + 127.0));
        }
        const uint32_t m_num = nk_clamp_uchar((float)ldg(k.m_num, j));
        const int n_id = ldg(k.n_id, j);
        const uint32_t n_kl = (n_id >= 0 && n_id < count) ? (uint32_t)n_id : 0xFFFFFFFFu;
        const uint8_t r[15] = {(uint8_t)qx, (uint8_t)(qx >> 8), (uint8_t)qy, (uint8_t)(qy >> 8), (uint8_t)rho, (uint8_t)(rho >> 8),
                               (uint8_t)s_rho, (uint8_t)(s_rho >> 8), (uint8_t)n_kl, (uint8_t)(n_kl >> 8), (uint8_t)(n_kl >> 16),
                               (uint8_t)(n_kl >> 24), (uint8_t)m_num, (uint8_t)fx, (uint8_t)fy};
        // the record's place relative to the workgroup's first word: -14 .. kNkBytes - 1
        const int at = 16 + (int)((long long)(lo + (size_t)j * 15) - (long long)w0);
#pragma unroll
        for (int i = 0; i < 15; i++) buf[at + i] = r[i];
    }
    __syncthreads();

    flush_words<uint8_t, kNkThreads>(buf + 16, a.rec, w0, kNkWords, b0, b1);
}

}  // namespace edgehip

using namespace edgehip;

struct edgehip_ctx::NetStore {
    int kl_size = 0;
    size_t rec_bytes = 0;              // nseq * kl_size * 15, rounded up to 16
    void *arena = nullptr;             // records | headers
    uint8_t *rec = nullptr;
    edgehip_net_header *hdr = nullptr;
    KProfStage k_prof;                 // edgehip_net_pack's argument on its way to the device
};

void edgehip::net_free(edgehip_ctx *c) {
    if (!c->net) return;
    (void)hipStreamSynchronize(c->stream);
    if (c->net->arena) (void)hipFree(c->net->arena);
    c->net->k_prof.destroy();
    delete c->net;
    c->net = nullptr;
}

bool edgehip::net_store(edgehip_ctx *c, const uint8_t **records, const edgehip_net_header **headers, int *kl_size) {
    if (!c->net) return false;
    *records = c->net->rec;
    *headers = c->net->hdr;
    *kl_size = c->net->kl_size;
    return true;
}

int edgehip_net_enable(edgehip_ctx *c, int kl_size) {
    EH_ENTER(c);
    if (kl_size < 0 || kl_size > EDGEHIP_KEYLINE_MAX) { set_error("net_enable: kl_size must be in [0, EDGEHIP_KEYLINE_MAX]"); return EDGEHIP_ERR_ARG; }
    net_free(c);
    if (kl_size == 0) return 0;
    auto *d = c->net = new edgehip_ctx::NetStore;
    const size_t B = c->plan.nseq;
    d->kl_size = kl_size;
    d->rec_bytes = (B * (size_t)kl_size * 15 + 15) & ~(size_t)15;
    const size_t bytes = d->rec_bytes + sizeof(edgehip_net_header) * B;
    if (hipMalloc(&d->arena, bytes) != hipSuccess || !d->k_prof.create(B)) {
        (void)hipGetLastError();
        net_free(c);
        set_error("net_enable: allocation failed");
        return EDGEHIP_ERR_MEMORY;
    }
    d->rec = (uint8_t *)d->arena;
    d->hdr = (edgehip_net_header *)(d->rec + d->rec_bytes);
    const hipError_t z = hipMemsetAsync(d->arena, 0, bytes, c->stream);
    if (z != hipSuccess) net_free(c);
    EH_CHECK(z);
    return 0;
}

int edgehip_net_pack(edgehip_ctx *c, int slot, int slot_pair, const double *k_prof) {
    EH_ENTER(c);
    if (slot < 0 || slot >= c->plan.nslots || slot_pair >= c->plan.nslots || slot_pair == slot) {
        set_error("net_pack: slot out of range (or the pair slot is the slot itself)");
        return EDGEHIP_ERR_ARG;
    }
    auto *d = c->net;
    if (!d) { set_error("net_pack: the record store is not enabled (edgehip_net_enable)"); return EDGEHIP_ERR_STATE; }
    const bool pair = slot_pair >= 0;
    if (pair && !klof(c, slot, 0).stereo_m_id) { set_error("net_pack: a pair slot needs params.stereo_available"); return EDGEHIP_ERR_STATE; }
    // the slot's KeyLines as edgehip_download_keylines returns them (see edgehip_depth_fill)
    if (int e = rot_materialize_enqueue(c, slot)) return e;
    if (pair) { if (int e = rot_materialize_enqueue(c, slot_pair)) return e; }
    if (int e = order_bc_after_a(c)) return e;
    if (k_prof) { if (int e = d->k_prof.push(c, k_prof)) return e; }
    NkArgs a;
    a.kls = kldev(c, slot);
    a.kls_pair = pair ? kldev(c, slot_pair) : nullptr;
    a.kns = c->kn_slot + (size_t)slot * c->plan.nseq;
    a.k_prof = k_prof ? d->k_prof.dev : nullptr;
    a.seqs = c->seq;
    a.rec = d->rec;
    a.hdr = d->hdr;
    a.kl_size = d->kl_size;
    a.cap = c->plan.cap;
    // words a sequence's records can span: its first word may start up to 15 B before its first byte
    const unsigned nblk = (unsigned)(((size_t)std::min(d->kl_size, c->plan.cap) * 15 + 15 + kNkBytes - 1) / kNkBytes);
    hipLaunchKernelGGL(k_net_pack, dim3(std::max(nblk, 1u), c->plan.nseq), dim3(kNkThreads), 0, c->stream, a);
    EH_LAUNCH_CHECK();
    // a later stage A that detects into these slots waits for the pack's reads
    if (int e = slot_read_done(c, slot)) return e;
    if (pair) { if (int e = slot_read_done(c, slot_pair)) return e; }
    return 0;
}

int edgehip_download_net_keylines_batch(edgehip_ctx *c, int n, const int32_t *seqs, edgehip_net_keyline *const *records,
                                        edgehip_net_header *const *headers) {
    EH_ENTER(c);
    auto *d = c->net;
    if (!d) { set_error("download_net_keylines: the record store is not enabled"); return EDGEHIP_ERR_STATE; }
    if (n < 1 || !seqs) { set_error("download_net_keylines: bad argument"); return EDGEHIP_ERR_ARG; }
    for (int j = 0; j < n; j++)
        if (seqs[j] < 0 || seqs[j] >= c->plan.nseq) { set_error("download_net_keylines: sequence out of range"); return EDGEHIP_ERR_ARG; }
    // the headers first (one copy): they say how many records exist
    std::vector<edgehip_net_header> h(c->plan.nseq);
    EH_CHECK(hipMemcpyAsync(h.data(), d->hdr, sizeof(edgehip_net_header) * h.size(), hipMemcpyDeviceToHost, c->stream));
    EH_CHECK(hipStreamSynchronize(c->stream));
    bool any = false;
    for (int j = 0; j < n; j++) {
        const int kn = std::max(0, std::min(h[seqs[j]].kline_num, d->kl_size));
        if (headers && headers[j]) *headers[j] = h[seqs[j]];
        if (records && records[j] && kn > 0) {
            EH_CHECK(hipMemcpyAsync(records[j], d->rec + (size_t)seqs[j] * d->kl_size * 15, (size_t)kn * 15, hipMemcpyDeviceToHost, c->stream));
            any = true;
        }
    }
    if (any) EH_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int edgehip_download_net_keylines(edgehip_ctx *c, int seq, edgehip_net_keyline *records, edgehip_net_header *header) {
    return edgehip_download_net_keylines_batch(c, 1, &seq, &records, &header);
}

int edgehip_net_keylines_device(edgehip_ctx *c, int first, int count, void *records_dev, void *headers_dev) {
    EH_ENTER(c);
    auto *d = c->net;
    if (!d) { set_error("net_keylines_device: the record store is not enabled"); return EDGEHIP_ERR_STATE; }
    if (first < 0 || count < 1 || first + count > c->plan.nseq) { set_error("net_keylines_device: sequence range out of bounds"); return EDGEHIP_ERR_ARG; }
    const size_t stride = (size_t)d->kl_size * 15;
    if (records_dev) EH_CHECK(hipMemcpyAsync(records_dev, d->rec + first * stride, stride * count, hipMemcpyDeviceToDevice, c->stream));
    if (headers_dev) EH_CHECK(hipMemcpyAsync(headers_dev, d->hdr + first, sizeof(edgehip_net_header) * count, hipMemcpyDeviceToDevice, c->stream));
    EH_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int edgehip_upload_net_keylines(edgehip_ctx *c, int seq, const edgehip_net_keyline *records, int32_t kn) {
    EH_ENTER(c);
    auto *d = c->net;
    if (!d) { set_error("upload_net_keylines: the record store is not enabled"); return EDGEHIP_ERR_STATE; }
    if (seq < 0 || seq >= c->plan.nseq) { set_error("upload_net_keylines: sequence out of range"); return EDGEHIP_ERR_ARG; }
    if (kn < 0 || kn > d->kl_size || (kn > 0 && !records)) { set_error("upload_net_keylines: kn exceeds kl_size, or null records"); return EDGEHIP_ERR_ARG; }
    const edgehip_net_header h = {kn, 0, 1.0f};
    if (kn > 0) EH_CHECK(hipMemcpyAsync(d->rec + (size_t)seq * d->kl_size * 15, records, (size_t)kn * 15, hipMemcpyHostToDevice, c->stream));
    EH_CHECK(hipMemcpyAsync(d->hdr + seq, &h, sizeof h, hipMemcpyHostToDevice, c->stream));
    EH_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}
