// ros_edgemap.hip — the per-frame output of the reference's ROS nodelet packed on the device: the loop of RebvoNodelet::edgeMapPubCb
// (ros/src/rebvo_ros/src/rebvo_nodelet.cpp:176-212) for every sequence of a slot in one launch.  Per KeyLine it builds one xyz float
// point, cam.unprojectHomCordVec(makeVector(p_m.x, p_m.y, rho / K)) (:203-208; include/UtilLib/cam_model.h:163-169), and one
// Keyline.msg record (:179-198).  The point's three values are fp64 quotients in the reference's order — the compiler's own IEEE
// division, scaling and fix-up included: rho reaches from 1e-300 to 1e35 here, far from the middle of the exponent range that ctx.h's
// shortened divisions assume — narrowed to float by v_cvt_f32_f64 (round to nearest even, float denormals kept).
//
// The hot part is the store.  Records are 12 and 52 bytes and a sequence's records start at seq * stride * 12 (52): a multiple of 4,
// not of 16.  A workgroup takes 256 consecutive KeyLines of one sequence (KeyLine j by lane j: the SoA reads are coalesced), i.e.
// 3072 and 13312 bytes of the two stores — both multiples of 16, so every workgroup of a sequence sees the same misalignment.  It
// lays its records out in LDS at the position they have relative to the 16-byte word that holds their first byte and writes the
// words out as 16-byte nontemporal stores.  With a misaligned sequence the first and the last word of a workgroup's bytes are shared
// with its neighbour (or, at the ends of the list, hold bytes that are not the sequence's): those two are written dword by dword,
// only the dwords that are the workgroup's own.  Nothing outside a sequence's kn records is ever written.
#include "ctx.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace edgehip {

constexpr int kRosThreads = 256;   // KeyLines per workgroup: 192 words of points, 832 words of records
constexpr int kRosPtBytes = kRosThreads * (int)sizeof(edgehip_ros_point);
constexpr int kRosKlBytes = kRosThreads * (int)sizeof(edgehip_ros_keyline);
static_assert(kRosPtBytes % 16 == 0 && kRosKlBytes % 16 == 0, "a workgroup's bytes are whole 16-byte words");

struct RosArgs {
    const KlSoA *kls;            // [nseq] KeyLines of the slot
    const int32_t *kns;          // [nseq]
    const int32_t *req;          // [gridDim.y] sequence of each list, or null: list j is sequence j
    const double *k_prof;        // [gridDim.y] or null: SeqDev::pub.K
    const SeqDev *seqs;          // [nseq]
    uint8_t *pts;                // [gridDim.y][stride][12] or null
    uint8_t *recs;               // [gridDim.y][stride][52] or null
    int32_t *kn_out;             // [gridDim.y] or null
    double zfm;
    int stride, cap;
};

// the workgroup's bytes [b0, b1) of a store, laid out in `buf` from offset (b0 & 15) on
__device__ __forceinline__ void ros_flush(const uint8_t *buf, uint8_t *store, const size_t b0, const size_t b1, const int tid) {
    typedef uint32_t u4v __attribute__((ext_vector_type(4)));
    const size_t w0 = b0 & ~(size_t)15;
    const int nw = (int)((b1 - w0 + 15) >> 4);
    for (int t = tid; t < nw; t += kRosThreads) {
        const size_t g = w0 + (size_t)t * 16;
        if (g >= b0 && g + 16 <= b1) {
            const u4v v = *reinterpret_cast<const u4v *>(buf + t * 16);
            __builtin_nontemporal_store(v, reinterpret_cast<u4v *>(store + g));
        } else {   // the first or the last word, partial: b0, b1 and g are multiples of 4
#pragma unroll
            for (int d = 0; d < 16; d += 4)
                if (g + d >= b0 && g + d < b1) *reinterpret_cast<uint32_t *>(store + g + d) = *reinterpret_cast<const uint32_t *>(buf + t * 16 + d);
        }
    }
}

__global__ __launch_bounds__(kRosThreads) void k_ros_pack(RosArgs a) {
    __shared__ __align__(16) uint8_t buf_p[16 + kRosPtBytes];
    __shared__ __align__(16) uint8_t buf_k[16 + kRosKlBytes];
    const int list = blockIdx.y, tid = threadIdx.x;
    const int seq = a.req ? a.req[list] : list;
    const int count = max(0, min(min(a.kns[seq], a.cap), a.stride));
    if (blockIdx.x == 0 && tid == 0 && a.kn_out) a.kn_out[list] = count;
    const int r0 = blockIdx.x * kRosThreads, r1 = min(r0 + kRosThreads, count);
    if (r0 >= count) return;
    const size_t lo_p = (size_t)list * a.stride * sizeof(edgehip_ros_point), lo_k = (size_t)list * a.stride * sizeof(edgehip_ros_keyline);
    const size_t p0 = lo_p + (size_t)r0 * sizeof(edgehip_ros_point), k0 = lo_k + (size_t)r0 * sizeof(edgehip_ros_keyline);

    const int j = r0 + tid;
    if (j < r1) {
        const KlSoA &k = a.kls[seq];
        const float2 pm = ldg(k.p_m, j);
        const double rho = ldg(k.rho, j);
        if (a.pts) {
            const double K = a.k_prof ? a.k_prof[list] : a.seqs[seq].pub.K;
            const double q = rho / K;
            const float x = (float)((double)pm.x / q / a.zfm);
            const float y = (float)((double)pm.y / q / a.zfm);
            const float z = (float)(1.0 / q);
            uint32_t *w = reinterpret_cast<uint32_t *>(buf_p + (p0 & 15) + tid * sizeof(edgehip_ros_point));
            w[0] = __float_as_uint(x); w[1] = __float_as_uint(y); w[2] = __float_as_uint(z);
        }
        if (a.recs) {
            const float2 mm = ldg(k.m_m, j), cp = ldg(k.c_p, j);
            const double s_rho = ldg(k.s_rho, j);
            const uint32_t p_id = (uint32_t)ldg(k.p_id, j), n_id = (uint32_t)ldg(k.n_id, j);
            uint32_t *w = reinterpret_cast<uint32_t *>(buf_k + (k0 & 15) + tid * sizeof(edgehip_ros_keyline));
            w[0] = __float_as_uint(mm.x); w[1] = __float_as_uint(mm.y);
            w[2] = __float_as_uint(cp.x); w[3] = __float_as_uint(cp.y);
            w[4] = (uint32_t)__double2loint(rho); w[5] = (uint32_t)__double2hiint(rho);
            w[6] = (uint32_t)__double2loint(s_rho); w[7] = (uint32_t)__double2hiint(s_rho);
            w[8] = __float_as_uint(pm.x); w[9] = __float_as_uint(pm.y);
            w[10] = (uint32_t)ldg(k.m_id, j);
            w[11] = (uint32_t)ldg(k.m_num, j);
            w[12] = (p_id & 0xFFFFu) | (n_id << 16);   // (int16_t)p_id, (int16_t)n_id: the low 16 bits of each
        }
    }
    __syncthreads();
    if (a.pts) ros_flush(buf_p, a.pts, p0, lo_p + (size_t)r1 * sizeof(edgehip_ros_point), tid);
    if (a.recs) ros_flush(buf_k, a.recs, k0, lo_k + (size_t)r1 * sizeof(edgehip_ros_keyline), tid);
}

static inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace edgehip

using namespace edgehip;

struct edgehip_ctx::RosStore {
    // ---- edgehip_ros_enable: the stores of the whole batch ----
    int what = 0;
    void *arena = nullptr;             // points | records | counts | k_prof
    uint8_t *pts = nullptr, *recs = nullptr;
    int32_t *kn = nullptr;             // [nseq]
    double *k_prof = nullptr;          // [nseq] device copy of edgehip_ros_pack's argument
    double *k_prof_host = nullptr;     // [nseq] page-locked staging of it
    hipEvent_t ev_k = nullptr;         // the last copy out of the staging has finished
    bool k_busy = false;
    // ---- edgehip_ros_export / _fetch / _wait: a staging ring of its own, like edgehip_ctx::KlExport ----
    static constexpr int R = 4;
    hipStream_t stream = nullptr;      // the copies to the host
    hipEvent_t ev_pack[R] = {}, ev_done[R] = {};
    int n_cap = 0, what_cap = 0;       // lists per entry and the record kinds the entries have room for
    size_t pts_bytes = 0, recs_bytes = 0;   // per entry, multiples of 16
    uint8_t *dev = nullptr;            // [R] entries of (points | records)
    int32_t *req = nullptr;            // page-locked [R][n_cap] sequence ids, read in place by the packing kernel
    double *req_k = nullptr;           // page-locked [R][n_cap] k_prof, likewise
    uint8_t *host[R] = {};             // page-locked mirror of an entry, allocated when a destination is not page-locked itself
    struct Staged { void *dst; const uint8_t *src; size_t bytes; };
    struct Ticket { long long id = -1; int n = 0, what = 0; bool fetched = false; std::vector<Staged> staged; } t[R];
    long long next = 0;
};

static void ros_stores_free(edgehip_ctx *c) {
    auto *d = c->ros;
    if (!d || !d->what) return;
    (void)hipStreamSynchronize(c->stream);
    if (d->arena) (void)hipFree(d->arena);
    if (d->k_prof_host) (void)hipHostFree(d->k_prof_host);
    if (d->ev_k) (void)hipEventDestroy(d->ev_k);
    d->arena = nullptr; d->pts = d->recs = nullptr; d->kn = nullptr; d->k_prof = nullptr; d->k_prof_host = nullptr; d->ev_k = nullptr;
    d->k_busy = false;
    d->what = 0;
}

static void ros_ring_free(edgehip_ctx::RosStore *d) {
    if (d->dev) (void)hipFree(d->dev);
    if (d->req) (void)hipHostFree(d->req);
    if (d->req_k) (void)hipHostFree(d->req_k);
    for (uint8_t *&h : d->host) if (h) { (void)hipHostFree(h); h = nullptr; }
    d->dev = nullptr; d->req = nullptr; d->req_k = nullptr;
    d->n_cap = 0; d->what_cap = 0;
}

void edgehip::ros_free(edgehip_ctx *c) {
    auto *d = c->ros;
    if (!d) return;
    ros_stores_free(c);
    (void)hipStreamSynchronize(c->stream);
    if (d->stream) { (void)hipStreamSynchronize(d->stream); (void)hipStreamDestroy(d->stream); }
    for (hipEvent_t e : d->ev_pack) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : d->ev_done) if (e) (void)hipEventDestroy(e);
    ros_ring_free(d);
    delete d;
    c->ros = nullptr;
}

int edgehip_ros_enable(edgehip_ctx *c, int what) {
    EH_ENTER(c);
    if (what & ~(EDGEHIP_ROS_POINTS | EDGEHIP_ROS_KEYLINES)) { set_error("ros_enable: what must be a combination of EDGEHIP_ROS_POINTS and EDGEHIP_ROS_KEYLINES"); return EDGEHIP_ERR_ARG; }
    ros_stores_free(c);
    if (what == 0) return 0;
    if (!c->ros) c->ros = new edgehip_ctx::RosStore;
    auto *d = c->ros;
    const size_t B = c->plan.nseq, cap = c->plan.cap;
    const size_t pb = (what & EDGEHIP_ROS_POINTS) ? up16(B * cap * sizeof(edgehip_ros_point)) : 0;
    const size_t kb = (what & EDGEHIP_ROS_KEYLINES) ? up16(B * cap * sizeof(edgehip_ros_keyline)) : 0;
    const size_t bytes = pb + kb + up16(4 * B) + 8 * B;
    void *arena = nullptr, *q = nullptr;
    hipEvent_t ev = nullptr;
    if (hipMalloc(&arena, bytes) != hipSuccess || hipHostMalloc(&q, 8 * B, hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        if (arena) (void)hipFree(arena);
        if (q) (void)hipHostFree(q);
        set_error("ros_enable: allocation failed");
        return EDGEHIP_ERR_MEMORY;
    }
    if (hipMemsetAsync(arena, 0, bytes, c->stream) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(arena);
        (void)hipHostFree(q);
        (void)hipEventDestroy(ev);
        set_error("ros_enable: hipMemsetAsync failed");
        return EDGEHIP_ERR_DEVICE;
    }
    d->arena = arena;
    d->pts = pb ? (uint8_t *)arena : nullptr;
    d->recs = kb ? (uint8_t *)arena + pb : nullptr;
    d->kn = (int32_t *)((uint8_t *)arena + pb + kb);
    d->k_prof = (double *)((uint8_t *)arena + pb + kb + up16(4 * B));
    d->k_prof_host = (double *)q;
    d->ev_k = ev;
    d->what = what;
    return 0;
}

static void ros_launch(edgehip_ctx *c, int slot, int nlists, const int32_t *req, const double *k_prof, uint8_t *pts, uint8_t *recs, int32_t *kn_out) {
    RosArgs a;
    a.kls = kldev(c, slot);
    a.kns = c->kn_slot + (size_t)slot * c->plan.nseq;
    a.req = req;
    a.k_prof = k_prof;
    a.seqs = c->seq;
    a.pts = pts;
    a.recs = recs;
    a.kn_out = kn_out;
    a.zfm = c->slot_cam[slot].zfm;
    a.stride = c->plan.cap;
    a.cap = c->plan.cap;
    const unsigned nblk = (unsigned)std::max(1, (c->plan.cap + kRosThreads - 1) / kRosThreads);
    hipLaunchKernelGGL(k_ros_pack, dim3(nblk, (unsigned)nlists), dim3(kRosThreads), 0, c->stream, a);
}

int edgehip_ros_pack(edgehip_ctx *c, int slot, const double *k_prof) {
    EH_ENTER(c);
    if (slot < 0 || slot >= c->plan.nslots) { set_error("ros_pack: slot out of range"); return EDGEHIP_ERR_ARG; }
    auto *d = c->ros;
    if (!d || !d->what) { set_error("ros_pack: the stores are not enabled (edgehip_ros_enable)"); return EDGEHIP_ERR_STATE; }
    // the slot's KeyLines as edgehip_download_keylines returns them (see edgehip_depth_fill)
    if (int e = rot_materialize_enqueue(c, slot)) return e;
    if (int e = order_bc_after_a(c)) return e;
    if (k_prof) {   // through the page-locked staging: the caller's array is free on return, and nothing waits for the stream
        if (d->k_busy) EH_CHECK(hipEventSynchronize(d->ev_k));   // (only for the copy of the pack before this one)
        memcpy(d->k_prof_host, k_prof, 8 * (size_t)c->plan.nseq);
        EH_CHECK(hipMemcpyAsync(d->k_prof, d->k_prof_host, 8 * (size_t)c->plan.nseq, hipMemcpyHostToDevice, c->stream));
        EH_CHECK(hipEventRecord(d->ev_k, c->stream));
        d->k_busy = true;
    }
    ros_launch(c, slot, c->plan.nseq, nullptr, k_prof ? d->k_prof : nullptr, d->pts, d->recs, d->kn);
    EH_LAUNCH_CHECK();
    if (c->stream_a != c->stream) {   // a later stage A that detects into this slot waits for the pack's reads
        EH_CHECK(hipEventRecord(c->ev_use[slot], c->stream));
        c->use_valid[slot] = true;
    }
    return 0;
}

int edgehip_download_ros_edgemaps_batch(edgehip_ctx *c, int n, const int32_t *seqs, edgehip_ros_point *const *points,
                                        edgehip_ros_keyline *const *keylines, int32_t *kn_out) {
    EH_ENTER(c);
    auto *d = c->ros;
    if (!d || !d->what) { set_error("download_ros_edgemap: the stores are not enabled"); return EDGEHIP_ERR_STATE; }
    if (n < 1 || !seqs) { set_error("download_ros_edgemap: bad argument"); return EDGEHIP_ERR_ARG; }
    for (int j = 0; j < n; j++)
        if (seqs[j] < 0 || seqs[j] >= c->plan.nseq) { set_error("download_ros_edgemap: sequence out of range"); return EDGEHIP_ERR_ARG; }
    // the counts first (one copy): they say how many records exist
    std::vector<int32_t> kn(c->plan.nseq);
    EH_CHECK(hipMemcpyAsync(kn.data(), d->kn, sizeof(int32_t) * kn.size(), hipMemcpyDeviceToHost, c->stream));
    EH_CHECK(hipStreamSynchronize(c->stream));
    const size_t cap = (size_t)c->plan.cap;
    bool any = false;
    for (int j = 0; j < n; j++) {
        const size_t k = (size_t)std::max(0, std::min(kn[seqs[j]], c->plan.cap));
        if (kn_out) kn_out[j] = (int32_t)k;
        if (k == 0) continue;
        if (d->pts && points && points[j]) {
            EH_CHECK(hipMemcpyAsync(points[j], d->pts + seqs[j] * cap * sizeof(edgehip_ros_point), k * sizeof(edgehip_ros_point), hipMemcpyDeviceToHost, c->stream));
            any = true;
        }
        if (d->recs && keylines && keylines[j]) {
            EH_CHECK(hipMemcpyAsync(keylines[j], d->recs + seqs[j] * cap * sizeof(edgehip_ros_keyline), k * sizeof(edgehip_ros_keyline), hipMemcpyDeviceToHost, c->stream));
            any = true;
        }
    }
    if (any) EH_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int edgehip_download_ros_edgemap(edgehip_ctx *c, int seq, edgehip_ros_point *points, edgehip_ros_keyline *keylines, int32_t *kn_out) {
    return edgehip_download_ros_edgemaps_batch(c, 1, &seq, &points, &keylines, kn_out);
}

int edgehip_ros_edgemap_device(edgehip_ctx *c, int first, int count, void *points_dev, void *keylines_dev, void *kn_dev) {
    EH_ENTER(c);
    auto *d = c->ros;
    if (!d || !d->what) { set_error("ros_edgemap_device: the stores are not enabled"); return EDGEHIP_ERR_STATE; }
    if (first < 0 || count < 1 || first + count > c->plan.nseq) { set_error("ros_edgemap_device: sequence range out of bounds"); return EDGEHIP_ERR_ARG; }
    if ((points_dev && !d->pts) || (keylines_dev && !d->recs)) { set_error("ros_edgemap_device: that store is not enabled"); return EDGEHIP_ERR_STATE; }
    const size_t sp = (size_t)c->plan.cap * sizeof(edgehip_ros_point), sk = (size_t)c->plan.cap * sizeof(edgehip_ros_keyline);
    if (points_dev) EH_CHECK(hipMemcpyAsync(points_dev, d->pts + first * sp, sp * count, hipMemcpyDeviceToDevice, c->stream));
    if (keylines_dev) EH_CHECK(hipMemcpyAsync(keylines_dev, d->recs + first * sk, sk * count, hipMemcpyDeviceToDevice, c->stream));
    if (kn_dev) EH_CHECK(hipMemcpyAsync(kn_dev, d->kn + first, sizeof(int32_t) * count, hipMemcpyDeviceToDevice, c->stream));
    EH_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int edgehip_ros_edgemap_from_device(edgehip_ctx *c, int first, int count, const void *points_dev, const void *keylines_dev) {
    EH_ENTER(c);
    auto *d = c->ros;
    if (!d || !d->what) { set_error("ros_edgemap_from_device: the stores are not enabled"); return EDGEHIP_ERR_STATE; }
    if (first < 0 || count < 1 || first + count > c->plan.nseq) { set_error("ros_edgemap_from_device: sequence range out of bounds"); return EDGEHIP_ERR_ARG; }
    if ((points_dev && !d->pts) || (keylines_dev && !d->recs)) { set_error("ros_edgemap_from_device: that store is not enabled"); return EDGEHIP_ERR_STATE; }
    const size_t sp = (size_t)c->plan.cap * sizeof(edgehip_ros_point), sk = (size_t)c->plan.cap * sizeof(edgehip_ros_keyline);
    if (points_dev) EH_CHECK(hipMemcpyAsync(d->pts + first * sp, points_dev, sp * count, hipMemcpyDeviceToDevice, c->stream));
    if (keylines_dev) EH_CHECK(hipMemcpyAsync(d->recs + first * sk, keylines_dev, sk * count, hipMemcpyDeviceToDevice, c->stream));
    EH_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

// ---- output callbacks at full pipeline depth: the ring of edgehip_export_keylines (api.hip) again, for the two small products ----
int edgehip_ros_export(edgehip_ctx *c, int n, const int32_t *seqs, const double *k_prof, int what, int *ticket_out) {
    EH_ENTER(c);
    if (n < 1 || !seqs || !k_prof || !ticket_out || !what || (what & ~(EDGEHIP_ROS_POINTS | EDGEHIP_ROS_KEYLINES))) {
        set_error("ros_export: bad argument (k_prof is required; what = EDGEHIP_ROS_POINTS | EDGEHIP_ROS_KEYLINES)");
        return EDGEHIP_ERR_ARG;
    }
    for (int j = 0; j < n; j++)
        if (seqs[j] < 0 || seqs[j] >= c->plan.nseq) { set_error("ros_export: sequence out of range"); return EDGEHIP_ERR_ARG; }
    if (c->frames_seen < 2 || c->frame_slot < 0) { set_error("ros_export: needs two processed frames (the old slot of a frame pair)"); return EDGEHIP_ERR_STATE; }
    if (!c->ros) c->ros = new edgehip_ctx::RosStore;
    auto *x = c->ros;
    constexpr int R = edgehip_ctx::RosStore::R;
    const size_t cap = (size_t)c->plan.cap;
    if (!x->stream) {
        EH_CHECK(hipStreamCreateWithFlags(&x->stream, hipStreamNonBlocking));
        for (int i = 0; i < R; i++) {
            EH_CHECK(hipEventCreateWithFlags(&x->ev_pack[i], hipEventDisableTiming));
            EH_CHECK(hipEventCreateWithFlags(&x->ev_done[i], hipEventDisableTiming));
        }
    }
    if (n > x->n_cap || (what & ~x->what_cap)) {   // room for n lists of these kinds per ticket (grown, never shrunk): only with no ticket outstanding
        for (auto &t : x->t)
            if (t.id >= 0) { set_error("ros_export: more lists (or another record kind) than before while tickets are outstanding"); return EDGEHIP_ERR_STATE; }
        EH_CHECK(hipStreamSynchronize(c->stream));
        EH_CHECK(hipStreamSynchronize(x->stream));
        const int n_new = std::max(n, x->n_cap), what_new = what | x->what_cap;
        ros_ring_free(x);
        x->pts_bytes = (what_new & EDGEHIP_ROS_POINTS) ? up16(cap * n_new * sizeof(edgehip_ros_point)) : 0;
        x->recs_bytes = (what_new & EDGEHIP_ROS_KEYLINES) ? up16(cap * n_new * sizeof(edgehip_ros_keyline)) : 0;
        void *q = nullptr;
        if (hipMalloc(&q, (x->pts_bytes + x->recs_bytes) * R) != hipSuccess) { (void)hipGetLastError(); set_error("ros_export: staging alloc failed"); return EDGEHIP_ERR_MEMORY; }
        x->dev = (uint8_t *)q;
        EH_CHECK(hipMemsetAsync(x->dev, 0, (x->pts_bytes + x->recs_bytes) * R, c->stream));
        if (hipHostMalloc(&q, sizeof(int32_t) * n_new * R, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); ros_ring_free(x); set_error("ros_export: pinned alloc failed"); return EDGEHIP_ERR_MEMORY; }
        x->req = (int32_t *)q;
        if (hipHostMalloc(&q, sizeof(double) * n_new * R, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); ros_ring_free(x); set_error("ros_export: pinned alloc failed"); return EDGEHIP_ERR_MEMORY; }
        x->req_k = (double *)q;
        x->n_cap = n_new;
        x->what_cap = what_new;
    }
    const int e = (int)(x->next % R);
    if (x->t[e].id >= 0) { set_error("ros_export: four tickets outstanding (edgehip_ros_export_wait releases one)"); return EDGEHIP_ERR_STATE; }
    const int so = (c->frame_slot - 1 + c->ring_slots) % c->ring_slots;
    if (int er = rot_materialize_enqueue(c, so)) return er;   // a slot the whole-frame driver rotated out of place (ctx.h: fuse_match)
    // (the entry's request rows are free: its last ticket was released behind its pack event, edgehip_ros_export_wait)
    int32_t *req = x->req + (size_t)e * x->n_cap;
    double *req_k = x->req_k + (size_t)e * x->n_cap;
    for (int j = 0; j < n; j++) { req[j] = seqs[j]; req_k[j] = k_prof[j]; }
    uint8_t *ent = x->dev + (size_t)e * (x->pts_bytes + x->recs_bytes);
    ros_launch(c, so, n, req, req_k, (what & EDGEHIP_ROS_POINTS) ? ent : nullptr, (what & EDGEHIP_ROS_KEYLINES) ? ent + x->pts_bytes : nullptr, nullptr);
    EH_LAUNCH_CHECK();
    EH_CHECK(hipEventRecord(x->ev_pack[e], c->stream));
    if (c->stream_a != c->stream) {   // the frame after next detects into this slot on the stage-A stream: not before the lists are out
        EH_CHECK(hipEventRecord(c->ev_use[so], c->stream));
        c->use_valid[so] = true;
    }
    x->t[e].id = x->next;
    x->t[e].n = n;
    x->t[e].what = what;
    x->t[e].fetched = false;
    x->t[e].staged.clear();
    *ticket_out = (int)(x->next & 0x7fffffff);
    x->next++;
    return 0;
}

static edgehip_ctx::RosStore::Ticket *ros_ticket(edgehip_ctx *c, int ticket, int &e) {
    auto *x = c->ros;
    if (!x) return nullptr;
    for (e = 0; e < edgehip_ctx::RosStore::R; e++)
        if (x->t[e].id >= 0 && (int)(x->t[e].id & 0x7fffffff) == ticket) return &x->t[e];
    return nullptr;
}

int edgehip_ros_export_fetch(edgehip_ctx *c, int ticket, const int32_t *kn, edgehip_ros_point *const *points_dst,
                             edgehip_ros_keyline *const *keylines_dst) {
    EH_ENTER(c);
    int e = 0;
    auto *t = ros_ticket(c, ticket, e);
    if (!t || !kn) { set_error("ros_export_fetch: unknown ticket or null argument"); return EDGEHIP_ERR_ARG; }
    if (t->fetched) { set_error("ros_export_fetch: ticket already fetched"); return EDGEHIP_ERR_STATE; }
    auto *x = c->ros;
    const size_t cap = (size_t)c->plan.cap, ent_bytes = x->pts_bytes + x->recs_bytes;
    for (int j = 0; j < t->n; j++)
        if (kn[j] < 0 || (size_t)kn[j] > cap) { set_error("ros_export_fetch: KeyLine count beyond the capacity"); return EDGEHIP_ERR_ARG; }
    // the page-locked mirror for pageable destinations first: once a copy is enqueued nothing below can fail for lack of memory
    for (int kind = 0; kind < 2 && !x->host[e]; kind++) {
        const int bit = kind ? EDGEHIP_ROS_KEYLINES : EDGEHIP_ROS_POINTS;
        const size_t rec = kind ? sizeof(edgehip_ros_keyline) : sizeof(edgehip_ros_point);
        for (int j = 0; j < t->n && !x->host[e]; j++) {
            const void *dst = kind ? (keylines_dst ? (const void *)keylines_dst[j] : nullptr) : (points_dst ? (const void *)points_dst[j] : nullptr);
            if (!(t->what & bit) || !dst || kn[j] <= 0 || host_range_registered(dst, (size_t)kn[j] * rec)) continue;
            void *q = nullptr;
            if (hipHostMalloc(&q, ent_bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); set_error("ros_export_fetch: pinned alloc failed"); return EDGEHIP_ERR_MEMORY; }
            x->host[e] = (uint8_t *)q;
        }
    }
    EH_CHECK(hipStreamWaitEvent(x->stream, x->ev_pack[e], 0));
    const uint8_t *ent = x->dev + (size_t)e * ent_bytes;
    t->staged.clear();
    for (int kind = 0; kind < 2; kind++) {
        const int bit = kind ? EDGEHIP_ROS_KEYLINES : EDGEHIP_ROS_POINTS;
        if (!(t->what & bit)) continue;
        const size_t rec = kind ? sizeof(edgehip_ros_keyline) : sizeof(edgehip_ros_point), base = kind ? x->pts_bytes : 0;
        for (int j = 0; j < t->n; j++) {
            void *dst = kind ? (keylines_dst ? (void *)keylines_dst[j] : nullptr) : (points_dst ? (void *)points_dst[j] : nullptr);
            if (!dst || kn[j] <= 0) continue;
            const size_t off = base + (size_t)j * cap * rec, bytes = (size_t)kn[j] * rec;
            void *to = dst;
            if (!host_range_registered(dst, bytes)) {
                // a pageable destination: through the page-locked mirror of the entry, and a host copy in edgehip_ros_export_wait
                to = x->host[e] + off;
                t->staged.push_back({dst, x->host[e] + off, bytes});
            }
            EH_CHECK(hipMemcpyAsync(to, ent + off, bytes, hipMemcpyDeviceToHost, x->stream));
        }
    }
    EH_CHECK(hipEventRecord(x->ev_done[e], x->stream));
    t->fetched = true;
    return 0;
}

int edgehip_ros_export_wait(edgehip_ctx *c, int ticket) {
    EH_ENTER(c);
    int e = 0;
    auto *t = ros_ticket(c, ticket, e);
    if (!t) { set_error("ros_export_wait: unknown ticket"); return EDGEHIP_ERR_ARG; }
    if (t->fetched) {
        EH_CHECK(hipEventSynchronize(c->ros->ev_done[e]));
        for (const auto &s : t->staged) memcpy(s.dst, s.src, s.bytes);
    } else {
        // never fetched: the packing kernel reads the entry's request rows in place and writes its staging, so the entry is free only
        // behind it — the next export into it may name other sequences
        EH_CHECK(hipEventSynchronize(c->ros->ev_pack[e]));
    }
    t->staged.clear();
    t->id = -1;
    t->fetched = false;
    return 0;
}
