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
// lays its records out in LDS at the position they have relative to the 16-byte word that holds their first byte, and flush_words
// (pack_flush.h) writes the words out.  With a misaligned sequence the first and the last word of a workgroup's bytes are shared with
// its neighbour (or, at the ends of the list, hold bytes that are not the sequence's).
#include "ctx.h"
#include "pack_flush.h"

#include <algorithm>
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
__device__ __forceinline__ void ros_flush(const uint8_t *buf, uint8_t *store, const size_t b0, const size_t b1) {
    const size_t w0 = b0 & ~(size_t)15;
    flush_words<uint32_t, kRosThreads>(buf, store, w0, (int)((b1 - w0 + 15) >> 4), b0, b1);
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
    if (a.pts) ros_flush(buf_p, a.pts, p0, lo_p + (size_t)r1 * sizeof(edgehip_ros_point));
    if (a.recs) ros_flush(buf_k, a.recs, k0, lo_k + (size_t)r1 * sizeof(edgehip_ros_keyline));
}

static inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace edgehip

using namespace edgehip;

struct edgehip_ctx::RosStore {
    // ---- edgehip_ros_enable: the stores of the whole batch ----
    int what = 0;
    void *arena = nullptr;             // points | records | counts
    uint8_t *pts = nullptr, *recs = nullptr;
    int32_t *kn = nullptr;             // [nseq]
    KProfStage k_prof;                 // edgehip_ros_pack's argument on its way to the device
    // ---- edgehip_ros_export: the record kinds the entries of edgehip_ctx::ros_ring have room for ----
    int what_cap = 0;
};

// an entry of the export ring: n_cap lists of points (when what_cap has them), then n_cap lists of records
static size_t ros_entry_pts_bytes(const edgehip_ctx *c, int what_cap, int n_cap) {
    return (what_cap & EDGEHIP_ROS_POINTS) ? up16((size_t)c->plan.cap * n_cap * sizeof(edgehip_ros_point)) : 0;
}

static void ros_stores_free(edgehip_ctx *c) {
    auto *d = c->ros;
    if (!d || !d->what) return;
    (void)hipStreamSynchronize(c->stream);
    if (d->arena) (void)hipFree(d->arena);
    d->k_prof.destroy();
    d->arena = nullptr; d->pts = d->recs = nullptr; d->kn = nullptr;
    d->what = 0;
}

void edgehip::ros_free(edgehip_ctx *c) {
    if (!c->ros) return;
    ros_stores_free(c);
    delete c->ros;
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
    const size_t bytes = pb + kb + 4 * B;
    d->what = what;   // (from here on ros_stores_free takes back whatever exists)
    if (hipMalloc(&d->arena, bytes) != hipSuccess || !d->k_prof.create(B)) {
        (void)hipGetLastError();
        ros_stores_free(c);
        set_error("ros_enable: allocation failed");
        return EDGEHIP_ERR_MEMORY;
    }
    d->pts = pb ? (uint8_t *)d->arena : nullptr;
    d->recs = kb ? (uint8_t *)d->arena + pb : nullptr;
    d->kn = (int32_t *)((uint8_t *)d->arena + pb + kb);
    const hipError_t z = hipMemsetAsync(d->arena, 0, bytes, c->stream);
    if (z != hipSuccess) ros_stores_free(c);
    EH_CHECK(z);
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
    if (k_prof) { if (int e = d->k_prof.push(c, k_prof)) return e; }
    ros_launch(c, slot, c->plan.nseq, nullptr, k_prof ? d->k_prof.dev : nullptr, d->pts, d->recs, d->kn);
    EH_LAUNCH_CHECK();
    return slot_read_done(c, slot);   // a later stage A that detects into this slot waits for the pack's reads
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

// ---- output callbacks at full pipeline depth, through c->ros_ring (export_ring.h), for the two small products ----
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
    ExportRing &x = c->ros_ring;
    if (int er = x.open(false)) return er;
    if (n > x.n_cap || (what & ~c->ros->what_cap)) {   // room for n lists of these kinds per entry
        const int n_new = std::max(n, x.n_cap), what_new = what | c->ros->what_cap;
        const size_t recs_bytes = (what_new & EDGEHIP_ROS_KEYLINES) ? (size_t)c->plan.cap * n_new * sizeof(edgehip_ros_keyline) : 0;
        if (int er = x.reserve(c, "ros_export", n_new, ros_entry_pts_bytes(c, what_new, n_new) + recs_bytes, (sizeof(double) + sizeof(int32_t)) * n_new)) return er;
        c->ros->what_cap = what_new;
    }
    int e = 0;
    if (int er = x.claim("ros_export", &e)) return er;
    const int so = (c->frame_slot - 1 + c->ring_slots) % c->ring_slots;
    if (int er = rot_materialize_enqueue(c, so)) return er;   // a slot the whole-frame driver rotated out of place (ctx.h: fuse_match)
    double *req_k = (double *)x.row(e);   // the entry's request row: k_prof, then the sequence ids
    int32_t *req = (int32_t *)(req_k + x.n_cap);
    for (int j = 0; j < n; j++) { req[j] = seqs[j]; req_k[j] = k_prof[j]; }
    uint8_t *ent = x.entry(e);
    ros_launch(c, so, n, req, req_k, (what & EDGEHIP_ROS_POINTS) ? ent : nullptr,
               (what & EDGEHIP_ROS_KEYLINES) ? ent + ros_entry_pts_bytes(c, c->ros->what_cap, x.n_cap) : nullptr, nullptr);
    EH_LAUNCH_CHECK();
    return x.commit(c, e, so, n, what, ticket_out);
}

int edgehip_ros_export_fetch(edgehip_ctx *c, int ticket, const int32_t *kn, edgehip_ros_point *const *points_dst,
                             edgehip_ros_keyline *const *keylines_dst) {
    EH_ENTER(c);
    int e = 0;
    ExportRing &x = c->ros_ring;
    auto *t = x.find(ticket, &e);
    if (!t || !kn) { set_error("ros_export_fetch: unknown ticket or null argument"); return EDGEHIP_ERR_ARG; }
    if (t->fetched) { set_error("ros_export_fetch: ticket already fetched"); return EDGEHIP_ERR_STATE; }
    const size_t cap = (size_t)c->plan.cap;
    for (int j = 0; j < t->n; j++)
        if (kn[j] < 0 || (size_t)kn[j] > cap) { set_error("ros_export_fetch: KeyLine count beyond the capacity"); return EDGEHIP_ERR_ARG; }
    std::vector<ExportRing::Copy> copies;
    for (int kind = 0; kind < 2; kind++) {
        const int bit = kind ? EDGEHIP_ROS_KEYLINES : EDGEHIP_ROS_POINTS;
        if (!(t->what & bit)) continue;
        const size_t rec = kind ? sizeof(edgehip_ros_keyline) : sizeof(edgehip_ros_point);
        const size_t base = kind ? ros_entry_pts_bytes(c, c->ros->what_cap, x.n_cap) : 0;
        for (int j = 0; j < t->n; j++) {
            void *dst = kind ? (keylines_dst ? (void *)keylines_dst[j] : nullptr) : (points_dst ? (void *)points_dst[j] : nullptr);
            if (dst && kn[j] > 0) copies.push_back({dst, base + (size_t)j * cap * rec, (size_t)kn[j] * rec});   // (a null destination is skipped)
        }
    }
    return x.fetch("ros_export_fetch", e, copies);
}

int edgehip_ros_export_wait(edgehip_ctx *c, int ticket) {
    EH_ENTER(c);
    int e = 0;
    if (!c->ros_ring.find(ticket, &e)) { set_error("ros_export_wait: unknown ticket"); return EDGEHIP_ERR_ARG; }
    return c->ros_ring.release(e);
}
