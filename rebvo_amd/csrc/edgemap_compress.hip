// edgemap_compress.hip — the reference's compressed edge map, edgemap_com_sender::compress_edgemap (src/CommLib/edgemap_com.cpp:162-326)
// with LineFitting::RobustFit3DLine<float> (src/UtilLib/linefitting.cpp:111-204), for every sequence of a slot.  The rule itself — one
// head's walk and the fit — is edgemap_fit.h, shared with the serial host restatement; this file is its parallel execution.
//
// The reference's loop is order dependent: heads (p_id < 0, mask bit clear) in ascending index, every walk setting and clearing bits of
// a shared mask.  But a walk reads and writes only KeyLines reachable from its head along n_id, so walks in different weakly connected
// components of the n_id graph commute, and only the heads of one component have to keep their order:
//   k_em_components  labels the components by their minimum index and sorts the heads' keys (label << 16 | index) — link_components.h,
//                    one workgroup per sequence, the keys in LDS up to 16384 KeyLines and in HBM above, the sorted keys left in HBM;
//   k_em_walk        one lane per component runs its heads serially, twice: a counting walk (no fits: no decision of the walk depends
//                    on one), an exclusive scan over the counts in index order — records are numbered in head order over the whole
//                    list —, then the walk with the fits, each head writing its records at its final numbers (8-byte scratch records);
//   k_em_place       packs them into the 5-byte store: a sequence's records start at seq * cap_records * 5, aligned to nothing, so the
//                    output is cut by address and written as 16-byte words through pack_flush.h, as k_net_pack does.
// The mask is 1 bit per KeyLine in LDS (atomic or / and: lanes of different components share words, never bits).
//
// Bounds by construction: links are read through link_in_range (anything outside [0, kn) is -1, and sets EDGEHIP_EDGEMAP_BAD_LINK), so
// every KeyLine index is below kn <= cap; a walk ends after at most kn + 1 steps; a record index is below the total of the scan, and
// nothing is written unless that total is at most cap_records (else count 0 and EDGEHIP_EDGEMAP_OVERFLOW).
#include "ctx.h"
#include "edgemap_fit.h"
#include "edgemap_seg.h"
#include "link_components.h"
#include "pack_flush.h"

#include <algorithm>
#include <cmath>
#include <vector>

static_assert(EDGEHIP_KEYLINE_MAX <= 65536, "component keys pack (label, index) into 16 + 16 bits; the mask has 65536 bits");

namespace edgehip {

namespace em = rebvo::edgemap;

constexpr int kEmCompThreads = 1024;     // k_em_components: one workgroup per sequence
constexpr int kEmLdsKeys = 16384;        // keys that fit 64 KB of LDS
constexpr int kEmWalkThreads = 256;      // k_em_walk: lanes (components in flight) per sequence
constexpr int kEmMaskWords = 65536 / 32;
constexpr int kEmPlaceThreads = 256;
constexpr int kEmWords = 240;            // 16-byte words per k_em_place workgroup: 3840 B = 768 records
constexpr int kEmBytes = kEmWords * 16;

struct EmArgs {
    const KlSoA *kls;         // [nseq] KeyLines of the slot
    const int32_t *kns;       // [nseq]
    const double *scale;      // [nseq] or null: 1
    uint32_t *keys;           // [nseq][np2cap] sorted head keys, 0xFFFFFFFF behind them
    uint32_t *offs;           // [nseq][cap] per KeyLine: a head's record count, then its first record number
    unsigned long long *tmp;  // [nseq][cap_records] records at their final numbers, unpacked
    uint8_t *rec;             // [nseq][cap_records][5]
    int32_t *count, *status;  // [nseq]
    float *rho_scale;         // [nseq] the scale the records were made with, as the reference keeps it (rho_scale=scale: narrowed to float)
    int cap, np2cap, cap_records;
    em::WalkParams P;         // (scale is filled per sequence)
};

struct SoaKeyLines {          // edgemap_fit.h's accessor over the device's structure of arrays
    const float2 *c_p, *u_m;
    const double *rho_, *s_rho_;
    const int32_t *m_num_, *p_id, *n_id;
    int n;
    __device__ int kn() const { return n; }
    __device__ int next(int k) const { return em::link_in_range(ldg(n_id, k), n); }
    __device__ int prev(int k) const { return em::link_in_range(ldg(p_id, k), n); }
    __device__ float cx(int k) const { return ldg(c_p, k).x; }
    __device__ float cy(int k) const { return ldg(c_p, k).y; }
    __device__ float ux(int k) const { return ldg(u_m, k).x; }
    __device__ float uy(int k) const { return ldg(u_m, k).y; }
    __device__ double rho(int k) const { return ldg(rho_, k); }
    __device__ double s_rho(int k) const { return ldg(s_rho_, k); }
    __device__ int m_num(int k) const { return ldg(m_num_, k); }
};
__device__ __forceinline__ SoaKeyLines em_keylines(const KlSoA &k, int kn) {
    return SoaKeyLines{k.c_p, k.u_m, k.rho, k.s_rho, k.m_num, k.p_id, k.n_id, kn};
}

struct LdsMask {              // kl_mask, 1 bit per KeyLine
    uint32_t *w;
    __device__ bool get(int k) const { return (__atomic_load_n(w + (k >> 5), __ATOMIC_RELAXED) >> (k & 31)) & 1u; }
    __device__ void set(int k) { atomicOr(w + (k >> 5), 1u << (k & 31)); }
    __device__ void clear(int k) { atomicAnd(w + (k >> 5), ~(1u << (k & 31))); }
};

struct TmpOut {               // a head's records at base + i of the sequence's scratch
    enum { kFit = 1 };
    unsigned long long *tmp;
    int base, cap;
    __device__ void put(int i, const em::Rec &r) {
        if (base + i < cap)
            tmp[base + i] = (unsigned long long)r.x | (unsigned long long)r.y << 8 | (unsigned long long)(uint16_t)r.rho << 16 |
                            (unsigned long long)r.s_rho << 32;
    }
};

// phase 0: labels, keys and sort in one launch.  A call made under edgehip_profile_enable launches it twice instead, so that the two stages
// can be timed apart: phase 1 stops behind the labelling and leaves the labels in the sequence's HBM keys, phase 2 takes them from there.
__global__ __launch_bounds__(kEmCompThreads) void k_em_components(EmArgs a, int phase) {
    extern __shared__ uint32_t em_lds[];
    __shared__ int changed;
    const int seq = blockIdx.x, tid = threadIdx.x;
    const int kn = max(0, min(a.kns[seq], a.cap));
    if (kn <= 0) return;
    const SoaKeyLines kl = em_keylines(a.kls[seq], kn);
    int np2 = 1;
    while (np2 < kn) np2 <<= 1;
    uint32_t *out = a.keys + (size_t)seq * a.np2cap;
    uint32_t *buf = np2 <= kEmLdsKeys ? em_lds : out;
    if (phase != 2) {
        lc_label_min<kEmCompThreads, 1>(buf, kn, &changed, [&](int i, int) { return kl.next(i); });
    } else if (buf != out) {
        for (int i = tid; i < kn; i += kEmCompThreads) buf[i] = out[i];
        __syncthreads();
    }
    if (phase == 1) {
        if (buf != out)
            for (int i = tid; i < kn; i += kEmCompThreads) out[i] = buf[i];
        return;
    }
    // keys of the heads; the others sort behind them
    int bad = 0;
    for (int i = tid; i < np2; i += kEmCompThreads) {
        uint32_t key = 0xFFFFFFFFu;
        if (i < kn) {
            const int p = ldg(kl.p_id, i), n = ldg(kl.n_id, i);
            bad |= em::link_is_bad(p, kn) || em::link_is_bad(n, kn);
            if (em::link_in_range(p, kn) < 0) key = buf[i] << 16 | (uint32_t)i;
        }
        buf[i] = key;
    }
    if (bad) atomicOr(a.status + seq, (int)em::kBadLink);
    __syncthreads();
    lc_sort<kEmCompThreads>(buf, np2);
    if (buf != out)
        for (int i = tid; i < kn; i += kEmCompThreads) out[i] = buf[i];
}

// one lane per component: its heads in ascending index
template <bool EMIT>
__device__ __forceinline__ void em_run_components(const EmArgs &a, const SoaKeyLines &kl, LdsMask &mask, const em::WalkParams &P, const uint32_t *keys,
                                                  uint32_t *offs, unsigned long long *tmp, int &status) {
    const int kn = kl.n;
    for (int k = threadIdx.x; k < kn; k += kEmWalkThreads) {
        const uint32_t key = keys[k];
        if (key == 0xFFFFFFFFu) break;   // (sorted: no heads from here on)
        const uint32_t lab = key >> 16;
        if (k > 0 && (keys[k - 1] >> 16) == lab) continue;
        for (int q = k; q < kn && (keys[q] >> 16) == lab; q++) {
            const int head = (int)(keys[q] & 0xFFFFu);
            if (mask.get(head)) continue;
            if (EMIT) {
                TmpOut o = {tmp, (int)offs[head], a.cap_records};
                (void)em::walk_head(kl, mask, P, head, o, status);
            } else {
                em::CountOnly o;
                offs[head] = (uint32_t)em::walk_head(kl, mask, P, head, o, status);
            }
        }
    }
}

__global__ __launch_bounds__(kEmWalkThreads) void k_em_walk(EmArgs a) {
    __shared__ uint32_t mask_w[kEmMaskWords];
    __shared__ uint32_t part[kEmWalkThreads];
    const int seq = blockIdx.x, tid = threadIdx.x;
    const int kn = max(0, min(a.kns[seq], a.cap));
    if (tid == 0) a.rho_scale[seq] = (float)(a.scale ? a.scale[seq] : 1.0);   // edgemap_com.cpp:322
    if (kn <= 0) {
        if (tid == 0) a.count[seq] = 0;
        return;
    }
    const SoaKeyLines kl = em_keylines(a.kls[seq], kn);
    const uint32_t *keys = a.keys + (size_t)seq * a.np2cap;
    uint32_t *offs = a.offs + (size_t)seq * a.cap;
    unsigned long long *tmp = a.tmp + (size_t)seq * a.cap_records;
    em::WalkParams P = a.P;
    P.scale = a.scale ? a.scale[seq] : 1.0;
    LdsMask mask = {mask_w};
    const int nw = (kn + 31) >> 5;
    for (int i = tid; i < nw; i += kEmWalkThreads) mask_w[i] = 0;
    for (int i = tid; i < kn; i += kEmWalkThreads) offs[i] = 0;
    __syncthreads();
    int status = 0;
    em_run_components<false>(a, kl, mask, P, keys, offs, tmp, status);
    __syncthreads();
    // exclusive scan of the counts in index order: thread t owns KeyLines [t * chunk, (t + 1) * chunk)
    const int chunk = (kn + kEmWalkThreads - 1) / kEmWalkThreads;
    const int lo = min(kn, tid * chunk), hi = min(kn, lo + chunk);
    uint32_t sum = 0;
    for (int i = lo; i < hi; i++) sum += offs[i];
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < kEmWalkThreads; d <<= 1) {
        const uint32_t v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    const uint32_t total = part[kEmWalkThreads - 1];
    uint32_t run = part[tid] - sum;
    for (int i = lo; i < hi; i++) {
        const uint32_t c = offs[i];
        offs[i] = run;
        run += c;
    }
    for (int i = tid; i < nw; i += kEmWalkThreads) mask_w[i] = 0;
    __syncthreads();
    if (total > (uint32_t)a.cap_records) {   // block-uniform
        if (status) atomicOr(a.status + seq, status);
        if (tid == 0) { a.count[seq] = 0; atomicOr(a.status + seq, (int)em::kOverflow); }
        return;
    }
    em_run_components<true>(a, kl, mask, P, keys, offs, tmp, status);
    if (status) atomicOr(a.status + seq, status);
    if (tid == 0) a.count[seq] = (int32_t)total;
}

__global__ __launch_bounds__(kEmPlaceThreads) void k_em_place(EmArgs a) {
    __shared__ __align__(16) uint8_t buf[16 + kEmBytes + 16];   // the workgroup's words at buf + 16; a shared record may start up to 4 B before them
    const int seq = blockIdx.y, tid = threadIdx.x;
    const int count = max(0, min(a.count[seq], a.cap_records));
    const size_t lo = (size_t)seq * a.cap_records * 5, hi = lo + (size_t)count * 5;
    const size_t w0 = (lo & ~(size_t)15) + (size_t)blockIdx.x * kEmBytes, w1 = w0 + kEmBytes;
    if (w0 >= hi) return;
    const size_t b0 = max(w0, lo), b1 = min(w1, hi);      // the bytes this workgroup writes
    const int r0 = (int)((b0 - lo) / 5), r1 = (int)((b1 - lo + 4) / 5);   // the records that touch them: at most 769
    const unsigned long long *tmp = a.tmp + (size_t)seq * a.cap_records;
    for (int j = r0 + tid; j < r1; j += kEmPlaceThreads) {
        const unsigned long long r = tmp[j];
        const int at = 16 + (int)((long long)(lo + (size_t)j * 5) - (long long)w0);   // -4 .. kEmBytes - 1 relative to the first word
#pragma unroll
        for (int i = 0; i < 5; i++) buf[at + i] = (uint8_t)(r >> (8 * i));
    }
    __syncthreads();
    flush_words<uint8_t, kEmPlaceThreads>(buf + 16, a.rec, w0, kEmWords, b0, b1);
}

// edgehip_edgemap_export: the record lists of the requested sequences, their counts and status words, into an entry of the export ring
// (lists at j * list_bytes, a multiple of 16; the (count, status) pairs behind them).  A sequence's records start at any byte: byte copies
// (a few thousand bytes per list).
__global__ __launch_bounds__(256) void k_em_gather(EmArgs a, const int32_t *__restrict__ req, uint8_t *__restrict__ lists, size_t list_bytes,
                                                   int32_t *__restrict__ pairs) {
    const int j = blockIdx.y, seq = req[j];
    const int count = max(0, min(a.count[seq], a.cap_records));
    if (blockIdx.x == 0 && threadIdx.x == 0) { pairs[2 * j] = count; pairs[2 * j + 1] = a.status[seq]; }
    const uint8_t *src = a.rec + (size_t)seq * a.cap_records * 5;
    uint8_t *dst = lists + (size_t)j * list_bytes;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)count * 5; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

}  // namespace edgehip

using namespace edgehip;

struct edgehip_ctx::EdgeMapStore {
    int cap_records = 0, np2cap = 1;
    size_t rec_bytes = 0;              // nseq * cap_records * 5, rounded up to 16
    std::vector<void *> dev;
    uint8_t *rec = nullptr;
    int32_t *count = nullptr, *status = nullptr;
    float *rho_scale = nullptr;
    uint32_t *keys = nullptr, *offs = nullptr;
    unsigned long long *tmp = nullptr;
    KProfStage scale;                  // edgehip_edgemap_compress's scale on its way to the device
    hipEvent_t ev_t[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // around the four stages of a call made under edgehip_profile_enable
    bool timed = false;
    size_t ring_list_bytes = 0;        // the list stride the entries of edgehip_ctx::em_ring were laid out with (0: not yet)
};

void edgehip::edgemap_free(edgehip_ctx *c) {
    auto *d = c->edgemap;
    if (!d) return;
    (void)hipStreamSynchronize(c->stream);
    for (void *q : d->dev) (void)hipFree(q);
    d->scale.destroy();
    for (hipEvent_t e : d->ev_t)
        if (e) (void)hipEventDestroy(e);
    delete d;
    c->edgemap = nullptr;
}

template <class T> static bool em_alloc(edgehip_ctx::EdgeMapStore *d, T **p, size_t count) {
    void *q = nullptr;
    if (hipMalloc(&q, sizeof(T) * std::max<size_t>(count, 1)) != hipSuccess) { (void)hipGetLastError(); return false; }
    d->dev.push_back(q);
    *p = (T *)q;
    return true;
}

int edgehip_edgemap_enable(edgehip_ctx *c, int cap_records) {
    EH_ENTER(c);
    if (cap_records < 0) { set_error("edgemap_enable: cap_records must be >= 0"); return EDGEHIP_ERR_ARG; }
    edgemap_free(c);
    if (cap_records == 0) return 0;
    // 64 KB of keys beside the kernel's own few bytes of LDS: opt in (the attribute belongs to the kernel, setting it again is harmless)
    EH_CHECK(hipFuncSetAttribute((const void *)&k_em_components, hipFuncAttributeMaxDynamicSharedMemorySize, kEmLdsKeys * (int)sizeof(uint32_t)));
    auto *d = c->edgemap = new edgehip_ctx::EdgeMapStore;
    const size_t B = c->plan.nseq, CAP = c->plan.cap;
    d->cap_records = cap_records;
    while ((size_t)d->np2cap < CAP) d->np2cap <<= 1;
    d->rec_bytes = (B * (size_t)cap_records * 5 + 15) & ~(size_t)15;
    bool ok = em_alloc(d, &d->rec, d->rec_bytes) && em_alloc(d, &d->count, B) && em_alloc(d, &d->status, B) && em_alloc(d, &d->rho_scale, B) &&
              em_alloc(d, &d->keys, B * (size_t)d->np2cap) && em_alloc(d, &d->offs, B * CAP) && em_alloc(d, &d->tmp, B * (size_t)cap_records) &&
              d->scale.create(B);
    for (hipEvent_t &e : d->ev_t) ok = ok && hipEventCreate(&e) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        edgemap_free(c);
        set_error("edgemap_enable: allocation failed");
        return EDGEHIP_ERR_MEMORY;
    }
    hipError_t z = hipMemsetAsync(d->rec, 0, d->rec_bytes, c->stream);
    if (z == hipSuccess) z = hipMemsetAsync(d->count, 0, sizeof(int32_t) * B, c->stream);
    if (z == hipSuccess) z = hipMemsetAsync(d->status, 0, sizeof(int32_t) * B, c->stream);
    // an empty store reads as made with scale 1 (edgemap_com's constructor): the bit pattern of 1.0f, in-stream like the rest
    if (z == hipSuccess) z = hipMemsetD32Async((hipDeviceptr_t)d->rho_scale, 0x3f800000, B, c->stream);
    if (z != hipSuccess) edgemap_free(c);
    EH_CHECK(z);
    return 0;
}

static int em_compress_enqueue(edgehip_ctx *c, int slot, const edgehip_edgemap_params *p, const double *scale, EmArgs *args_out);

int edgehip_edgemap_compress(edgehip_ctx *c, int slot, const edgehip_edgemap_params *p, const double *scale) {
    EH_ENTER(c);
    return em_compress_enqueue(c, slot, p, scale, nullptr);
}

static int em_compress_enqueue(edgehip_ctx *c, int slot, const edgehip_edgemap_params *p, const double *scale, EmArgs *args_out) {
    auto *d = c->edgemap;
    if (!d) { set_error("edgemap_compress: the record store is not enabled (edgehip_edgemap_enable)"); return EDGEHIP_ERR_STATE; }
    if (slot < 0 || slot >= c->plan.nslots) { set_error("edgemap_compress: slot out of range"); return EDGEHIP_ERR_ARG; }
    if (!p || p->min_line_len < 0 || p->max_line_len < 1 || !(p->x_scaling >= 0) || !(p->y_scaling >= 0)) {
        set_error("edgemap_compress: min_line_len >= 0, max_line_len >= 1 and scalings >= 0 are required");
        return EDGEHIP_ERR_ARG;
    }
    // the slot's KeyLines as edgehip_download_keylines returns them (see edgehip_depth_fill)
    if (int e = rot_materialize_enqueue(c, slot)) return e;
    if (int e = order_bc_after_a(c)) return e;
    if (scale) { if (int e = d->scale.push(c, scale)) return e; }
    EmArgs a;
    a.kls = kldev(c, slot);
    a.kns = c->kn_slot + (size_t)slot * c->plan.nseq;
    a.scale = scale ? d->scale.dev : nullptr;
    a.keys = d->keys; a.offs = d->offs; a.tmp = d->tmp; a.rec = d->rec; a.count = d->count; a.status = d->status;
    a.rho_scale = d->rho_scale;
    a.cap = c->plan.cap; a.np2cap = d->np2cap; a.cap_records = d->cap_records;
    a.P.min_line_len = p->min_line_len; a.P.max_line_len = p->max_line_len; a.P.match_n_t = p->match_n_t;
    a.P.max_cangle = std::cos(p->max_angle);
    a.P.rho_rel_max = p->rho_rel_max;
    a.P.x_scaling = p->x_scaling == 0 ? 0.5 : p->x_scaling;
    a.P.y_scaling = p->y_scaling == 0 ? 1.0 : p->y_scaling;
    a.P.scale = 1.0;
    a.P.ppx = c->plan.ppx; a.P.ppy = c->plan.ppy; a.P.zfm = c->plan.zfm;
    const int B = c->plan.nseq;
    d->timed = c->prof->on;
    EH_CHECK(hipMemsetAsync(d->status, 0, sizeof(int32_t) * (size_t)B, c->stream));
    if (d->timed) EH_CHECK(hipEventRecord(d->ev_t[0], c->stream));
    const size_t lds = sizeof(uint32_t) * (size_t)std::min(d->np2cap, kEmLdsKeys);
    if (d->timed) {   // labelling and sort as two launches, an event between them (the labels cross in HBM)
        hipLaunchKernelGGL(k_em_components, dim3(B), dim3(kEmCompThreads), lds, c->stream, a, 1);
        EH_LAUNCH_CHECK();
        EH_CHECK(hipEventRecord(d->ev_t[1], c->stream));
        hipLaunchKernelGGL(k_em_components, dim3(B), dim3(kEmCompThreads), lds, c->stream, a, 2);
        EH_LAUNCH_CHECK();
        EH_CHECK(hipEventRecord(d->ev_t[2], c->stream));
    } else {
        hipLaunchKernelGGL(k_em_components, dim3(B), dim3(kEmCompThreads), lds, c->stream, a, 0);
        EH_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_em_walk, dim3(B), dim3(kEmWalkThreads), 0, c->stream, a);
    EH_LAUNCH_CHECK();
    if (d->timed) EH_CHECK(hipEventRecord(d->ev_t[3], c->stream));
    const unsigned nblk = (unsigned)(((size_t)d->cap_records * 5 + 15 + kEmBytes - 1) / kEmBytes);
    hipLaunchKernelGGL(k_em_place, dim3(std::max(nblk, 1u), B), dim3(kEmPlaceThreads), 0, c->stream, a);
    EH_LAUNCH_CHECK();
    if (d->timed) EH_CHECK(hipEventRecord(d->ev_t[4], c->stream));
    if (args_out) *args_out = a;
    // a later stage A that detects into the slot waits for these reads
    return slot_read_done(c, slot);
}

static size_t em_list_bytes(const edgehip_ctx *c) { return ((size_t)c->edgemap->cap_records * 5 + 15) & ~(size_t)15; }

int edgehip_edgemap_export(edgehip_ctx *c, int n, const int32_t *seqs, const double *scale, const edgehip_edgemap_params *p, int *ticket_out) {
    EH_ENTER(c);
    if (!c->edgemap) { set_error("edgemap_export: the record store is not enabled (edgehip_edgemap_enable)"); return EDGEHIP_ERR_STATE; }
    if (n < 1 || !seqs || !scale || !ticket_out) { set_error("edgemap_export: bad argument (scale is required)"); return EDGEHIP_ERR_ARG; }
    for (int j = 0; j < n; j++)
        if (seqs[j] < 0 || seqs[j] >= c->plan.nseq) { set_error("edgemap_export: sequence out of range"); return EDGEHIP_ERR_ARG; }
    if (c->frames_seen < 2 || c->frame_slot < 0) { set_error("edgemap_export: needs two processed frames (the old slot of a frame pair)"); return EDGEHIP_ERR_STATE; }
    ExportRing &x = c->em_ring;
    if (int er = x.open(false)) return er;
    const size_t lb = em_list_bytes(c);
    if (n > x.n_cap || c->edgemap->ring_list_bytes != lb) {   // room for n lists of this store's size per entry
        const int n_new = std::max(n, x.n_cap);
        if (int er = x.reserve(c, "edgemap_export", n_new, (lb + 8) * (size_t)n_new, sizeof(int32_t) * (size_t)n_new)) return er;
        c->edgemap->ring_list_bytes = lb;
    }
    int e = 0;
    if (int er = x.claim("edgemap_export", &e)) return er;
    const int so = (c->frame_slot - 1 + c->ring_slots) % c->ring_slots;
    std::vector<double> all((size_t)c->plan.nseq, 1.0);
    for (int j = 0; j < n; j++) all[seqs[j]] = scale[j];
    EmArgs a;
    if (int er = em_compress_enqueue(c, so, p, all.data(), &a)) return er;
    int32_t *req = (int32_t *)x.row(e);
    for (int j = 0; j < n; j++) req[j] = seqs[j];
    uint8_t *ent = x.entry(e);
    const unsigned nblk = (unsigned)std::min<size_t>(16, (lb + 256 * 16 - 1) / (256 * 16));
    hipLaunchKernelGGL(k_em_gather, dim3(std::max(nblk, 1u), n), dim3(256), 0, c->stream, a, (const int32_t *)req, ent, lb, (int32_t *)(ent + lb * x.n_cap));
    EH_LAUNCH_CHECK();
    return x.commit(c, e, so, n, 0, ticket_out);
}

int edgehip_edgemap_export_fetch(edgehip_ctx *c, int ticket, const int32_t *max_records, edgehip_compressed_kl *const *records_dst, int32_t *pairs_dst) {
    EH_ENTER(c);
    int e = 0;
    ExportRing &x = c->em_ring;
    auto *t = x.find(ticket, &e);
    if (!t || !max_records || !pairs_dst || !c->edgemap) { set_error("edgemap_export_fetch: unknown ticket or null argument"); return EDGEHIP_ERR_ARG; }
    if (t->fetched) { set_error("edgemap_export_fetch: ticket already fetched"); return EDGEHIP_ERR_STATE; }
    const size_t lb = em_list_bytes(c);
    if (c->edgemap->ring_list_bytes != lb) { set_error("edgemap_export_fetch: the store was resized since the export"); return EDGEHIP_ERR_STATE; }
    std::vector<ExportRing::Copy> copies;
    for (int j = 0; j < t->n; j++) {
        if (max_records[j] < 0) { set_error("edgemap_export_fetch: negative max_records"); return EDGEHIP_ERR_ARG; }
        const size_t k = std::min<size_t>((size_t)max_records[j], (size_t)c->edgemap->cap_records);
        if (records_dst && records_dst[j] && k > 0) copies.push_back({(void *)records_dst[j], (size_t)j * lb, k * 5});
    }
    copies.push_back({(void *)pairs_dst, lb * x.n_cap, sizeof(int32_t) * 2 * (size_t)t->n});
    return x.fetch("edgemap_export_fetch", e, copies);
}

int edgehip_edgemap_export_wait(edgehip_ctx *c, int ticket) {
    EH_ENTER(c);
    int e = 0;
    if (!c->em_ring.find(ticket, &e)) { set_error("edgemap_export_wait: unknown ticket"); return EDGEHIP_ERR_ARG; }
    return c->em_ring.release(e);
}

int edgehip_download_edgemap_batch(edgehip_ctx *c, int n, const int32_t *seqs, edgehip_compressed_kl *const *records, int32_t *counts,
                                   int32_t *status) {
    EH_ENTER(c);
    auto *d = c->edgemap;
    if (!d) { set_error("download_edgemap: the record store is not enabled"); return EDGEHIP_ERR_STATE; }
    if (n < 1 || !seqs) { set_error("download_edgemap: bad argument"); return EDGEHIP_ERR_ARG; }
    for (int j = 0; j < n; j++)
        if (seqs[j] < 0 || seqs[j] >= c->plan.nseq) { set_error("download_edgemap: sequence out of range"); return EDGEHIP_ERR_ARG; }
    // the counts first (one copy): they say how many records exist
    std::vector<int32_t> cs(2 * (size_t)c->plan.nseq);
    EH_CHECK(hipMemcpyAsync(cs.data(), d->count, sizeof(int32_t) * c->plan.nseq, hipMemcpyDeviceToHost, c->stream));
    EH_CHECK(hipMemcpyAsync(cs.data() + c->plan.nseq, d->status, sizeof(int32_t) * c->plan.nseq, hipMemcpyDeviceToHost, c->stream));
    EH_CHECK(hipStreamSynchronize(c->stream));
    bool any = false;
    for (int j = 0; j < n; j++) {
        const int k = std::max(0, std::min(cs[seqs[j]], d->cap_records));
        if (counts) counts[j] = k;
        if (status) status[j] = cs[c->plan.nseq + seqs[j]];
        if (records && records[j] && k > 0) {
            EH_CHECK(hipMemcpyAsync(records[j], d->rec + (size_t)seqs[j] * d->cap_records * 5, (size_t)k * 5, hipMemcpyDeviceToHost, c->stream));
            any = true;
        }
    }
    if (any) EH_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int edgehip_download_edgemap(edgehip_ctx *c, int seq, edgehip_compressed_kl *records, int32_t *count, int32_t *status) {
    return edgehip_download_edgemap_batch(c, 1, &seq, &records, count, status);
}

bool edgehip::edgemap_store(edgehip_ctx *c, const uint8_t **records, const int32_t **counts, const float **rho_scale, int *cap_records) {
    auto *d = c->edgemap;
    if (!d) return false;
    *records = d->rec; *counts = d->count; *rho_scale = d->rho_scale; *cap_records = d->cap_records;
    return true;
}

int edgehip_upload_edgemap(edgehip_ctx *c, int seq, const edgehip_compressed_kl *records, int32_t count, float rho_scale) {
    EH_ENTER(c);
    auto *d = c->edgemap;
    if (!d) { set_error("upload_edgemap: the record store is not enabled (edgehip_edgemap_enable)"); return EDGEHIP_ERR_STATE; }
    if (seq < 0 || seq >= c->plan.nseq) { set_error("upload_edgemap: sequence out of range"); return EDGEHIP_ERR_ARG; }
    if (count < 0 || count > d->cap_records || (count > 0 && !records)) { set_error("upload_edgemap: count outside [0, cap_records], or null records"); return EDGEHIP_ERR_ARG; }
    // getPair divides rho by COMPRESSED_RHO_SCALING / rho_scale: that quotient has to be a finite positive float (rho_scale above
    // about 5e-36), or every rho becomes +-0 and the walk's `kl1.rho < 0` no longer sees a closing record
    if (!std::isfinite(rho_scale) || !(rho_scale > 0) || !std::isfinite(em::kSegRhoScaling / rho_scale)) {
        set_error("upload_edgemap: rho_scale must be finite, > 0 and large enough that (32767 / 20) / rho_scale is a finite float");
        return EDGEHIP_ERR_ARG;
    }
    const int32_t zero = 0;
    if (count > 0) EH_CHECK(hipMemcpyAsync(d->rec + (size_t)seq * d->cap_records * 5, records, (size_t)count * 5, hipMemcpyHostToDevice, c->stream));
    EH_CHECK(hipMemcpyAsync(d->count + seq, &count, sizeof count, hipMemcpyHostToDevice, c->stream));
    EH_CHECK(hipMemcpyAsync(d->status + seq, &zero, sizeof zero, hipMemcpyHostToDevice, c->stream));
    EH_CHECK(hipMemcpyAsync(d->rho_scale + seq, &rho_scale, sizeof rho_scale, hipMemcpyHostToDevice, c->stream));
    EH_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int edgehip_edgemap_device(edgehip_ctx *c, int first, int count, void *records_dev, void *counts_dev) {
    EH_ENTER(c);
    auto *d = c->edgemap;
    if (!d) { set_error("edgemap_device: the record store is not enabled"); return EDGEHIP_ERR_STATE; }
    if (first < 0 || count < 1 || first + count > c->plan.nseq) { set_error("edgemap_device: sequence range out of bounds"); return EDGEHIP_ERR_ARG; }
    const size_t stride = (size_t)d->cap_records * 5;
    if (records_dev) EH_CHECK(hipMemcpyAsync(records_dev, d->rec + first * stride, stride * count, hipMemcpyDeviceToDevice, c->stream));
    if (counts_dev) EH_CHECK(hipMemcpyAsync(counts_dev, d->count + first, sizeof(int32_t) * count, hipMemcpyDeviceToDevice, c->stream));
    EH_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int edgehip_edgemap_ms(edgehip_ctx *c, float ms[4]) {
    EH_ENTER(c);
    auto *d = c->edgemap;
    if (!d || !d->timed || !ms) { set_error("edgemap_ms: the last edgehip_edgemap_compress was not made under edgehip_profile_enable"); return EDGEHIP_ERR_STATE; }
    EH_CHECK(hipEventSynchronize(d->ev_t[4]));
    for (int i = 0; i < 4; i++) EH_CHECK(hipEventElapsedTime(ms + i, d->ev_t[i], d->ev_t[i + 1]));
    return 0;
}
