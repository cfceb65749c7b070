// edgemap_decode.hip — the receiving side of the compressed edge map, edgemap_com_decoder (include/CommLib/edgemap_com.h:226-252,
// src/CommLib/edgemap_com.cpp:42-160, 431-528), for every sequence of a context.  The rules themselves — which record starts a segment,
// how a record becomes a point, TransformPos, fillDepthMap's gates and steps — are edgemap_seg.h, shared with the serial host
// restatement (rebvo/edgemap_com.h); this file is their parallel execution over the record store of edgemap_compress.hip.
//
//   k_em_decode   one workgroup per sequence: one flag per record (does it start a segment), an exclusive scan of the flags, and
//                 segment j written at j — record order, which is the order getPair's cursor finds them in.  The list is cut at
//                 cap_segments in that order (Decode's seg_num < KEYLINE_MAX).
//   k_em_hide     one lane per segment of every sequence: TransformPos on both end points and HideVisible's frame test; a wave's
//                 survivors are counted with one ballot and one atomic.
//   k_em_items    one workgroup per sequence: fillDepthMap's gates and step count of every segment, the direction and per-step
//                 constants of those that have steps, and an exclusive scan of the step counts: the (segment, step) items the segment
//                 source of k_depth_fill (depth_fill.hip) bins and folds.  More than cap_items items: a status bit and no item.
//
// Bounds by construction: a record index is below min(count, cap_records); a segment index is below min(scan total, cap_segments); the
// step counts are clamped to cap_items + 1 and their sums saturate there, so no sum overflows and an item number is below cap_items.
#include "ctx.h"
#include "edgemap_seg.h"

#include <cmath>
#include <vector>

namespace edgehip {

namespace em = rebvo::edgemap;

constexpr int kEdThreads = 256;

struct EdArgs {
    const uint8_t *rec;         // [nseq][cap_records][5]
    const int32_t *count;       // [nseq]
    const float *rho_scale;     // [nseq]
    float *seg;                 // [nseq][cap_segments][8]
    uint8_t *flag;              // [nseq][cap_segments]
    int32_t *seg_num, *status;  // [nseq]
    int32_t *seg_off;           // [nseq][cap_segments + 1]
    double *seg_dir;            // [nseq][cap_segments][4]
    int32_t *items;             // [nseq]
    const double *pose;         // [nseq][16] DPose[9], DPos[3], k_em, k_new, active, unused
    int32_t *s_num;             // [nseq]
    int cap_records, cap_segments, cap_items;
    double x_scaling, y_scaling, v_thresh, cos_a;
    int use_visibility;
    em::SegCam cam;
};

struct EdRec { int x, y, rho, s_rho; };
__device__ __forceinline__ EdRec ed_rec(const uint8_t *rec, int i) {   // byte loads: a record is aligned to nothing
    const uint8_t *p = rec + (size_t)i * 5;
    EdRec r;
    r.x = ldg(p, 0);
    r.y = ldg(p, 1);
    r.rho = (int16_t)(ldg(p, 2) | (ldg(p, 3) << 8));
    r.s_rho = ldg(p, 4);
    return r;
}
__device__ __forceinline__ int ed_rho(const uint8_t *rec, int i) { return (int16_t)(ldg(rec, (size_t)i * 5 + 2) | (ldg(rec, (size_t)i * 5 + 3) << 8)); }

// inclusive scan of one value per thread over the workgroup (part: kEdThreads ints); sat > 0: sums saturate at sat
__device__ __forceinline__ int ed_scan(int32_t *part, int tid, int v, int sat) {
    part[tid] = v;
    __syncthreads();
    for (int d = 1; d < kEdThreads; d <<= 1) {
        const int u = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] = sat > 0 ? min(part[tid] + u, sat) : part[tid] + u;
        __syncthreads();
    }
    return part[tid];
}

__global__ __launch_bounds__(kEdThreads) void k_em_decode(EdArgs a) {
    __shared__ int32_t part[kEdThreads];
    const int seq = blockIdx.x, tid = threadIdx.x;
    const int n = max(0, min(a.count[seq], a.cap_records));
    const uint8_t *rec = a.rec + (size_t)seq * a.cap_records * 5;
    const float rho_scale = a.rho_scale[seq];
    float *seg = a.seg + (size_t)seq * a.cap_segments * 8;
    uint8_t *flag = a.flag + (size_t)seq * a.cap_segments;
    // thread t owns the records [lo, hi): flags, then their numbers
    const int chunk = (n + kEdThreads - 1) / kEdThreads;
    const int lo = min(n, tid * chunk), hi = min(n, lo + chunk);
    int sum = 0;
    for (int i = lo; i < hi; i++) sum += em::seg_starts(i >= 1 ? ed_rho(rec, i - 1) : 0, ed_rho(rec, i), i, n) ? 1 : 0;
    const int incl = ed_scan(part, tid, sum, 0);
    const int total = part[kEdThreads - 1];
    int j = incl - sum;
    for (int i = lo; i < hi && j < a.cap_segments; i++) {
        const EdRec r0 = ed_rec(rec, i);
        if (!em::seg_starts(i >= 1 ? ed_rho(rec, i - 1) : 0, r0.rho, i, n)) continue;
        const EdRec r1 = ed_rec(rec, i + 1);   // i < n - 1
        em::SegPoint k0, k1;
        em::seg_pair(r0.x, r0.y, r0.rho, r0.s_rho, r1.x, r1.y, r1.rho, r1.s_rho, rho_scale, a.x_scaling, a.y_scaling, &k0, &k1);
        float *o = seg + (size_t)j * 8;
        o[0] = k0.x; o[1] = k0.y; o[2] = k0.rho; o[3] = k0.s_rho;
        o[4] = k1.x; o[5] = k1.y; o[6] = k1.rho; o[7] = k1.s_rho;
        flag[j] = 1;
        j++;
    }
    if (tid == 0) {
        a.seg_num[seq] = min(total, a.cap_segments);
        a.status[seq] = total > a.cap_segments ? EDGEHIP_EDGEMAP_SEGMENT_OVERFLOW : 0;
        a.items[seq] = 0;
    }
}

__device__ __forceinline__ void ed_seg(const float *seg, int j, em::SegPoint *k0, em::SegPoint *k1) {
    const float4 p0 = ldg((const float4 *)seg, (size_t)2 * j), p1 = ldg((const float4 *)seg, (size_t)2 * j + 1);
    k0->x = p0.x; k0->y = p0.y; k0->rho = p0.z; k0->s_rho = p0.w;
    k1->x = p1.x; k1->y = p1.y; k1->rho = p1.z; k1->s_rho = p1.w;
}

__global__ __launch_bounds__(kEdThreads) void k_em_hide(EdArgs a) {
    const int seq = blockIdx.y, j = blockIdx.x * kEdThreads + threadIdx.x;
    const double *P = a.pose + (size_t)seq * 16;
    if (P[14] == 0) return;                               // a NULL row: this sequence is left alone (block-uniform)
    const int n = min(a.seg_num[seq], a.cap_segments);
    bool keep = false;
    if (j < n) {
        uint8_t *flag = a.flag + (size_t)seq * a.cap_segments;
        if (flag[j]) {
            em::SegPoint k0, k1;
            ed_seg(a.seg + (size_t)seq * a.cap_segments * 8, j, &k0, &k1);
            if (em::seg_seen(k0, k1, P, P + 9, (float)P[12], (float)P[13], a.cam)) flag[j] = 0;
            else keep = true;
        }
    }
    const unsigned long long b = __ballot(keep);
    if ((threadIdx.x & (warpSize - 1)) == 0 && b) atomicAdd(a.s_num + seq, __popcll(b));
}

__global__ __launch_bounds__(kEdThreads) void k_em_items(EdArgs a) {
    __shared__ int32_t part[kEdThreads];
    const int seq = blockIdx.x, tid = threadIdx.x;
    const int n = max(0, min(a.seg_num[seq], a.cap_segments));
    const float *seg = a.seg + (size_t)seq * a.cap_segments * 8;
    const uint8_t *flag = a.flag + (size_t)seq * a.cap_segments;
    int32_t *off = a.seg_off + (size_t)seq * (a.cap_segments + 1);
    double *dir = a.seg_dir + (size_t)seq * a.cap_segments * 4;
    const int sat = a.cap_items + 1;
    const int chunk = (n + kEdThreads - 1) / kEdThreads;
    const int lo = min(n, tid * chunk), hi = min(n, lo + chunk);
    int sum = 0;
    for (int j = lo; j < hi; j++) {
        int steps = 0;
        if (!a.use_visibility || flag[j]) {
            em::SegPoint k0, k1;
            ed_seg(seg, j, &k0, &k1);
            const em::SegSteps s = em::seg_steps(k0, k1, a.cam, a.v_thresh, a.cos_a, nullptr);
            steps = min(s.n, sat);
            if (steps > 0) { dir[4 * j] = s.tx; dir[4 * j + 1] = s.ty; dir[4 * j + 2] = s.r1; dir[4 * j + 3] = s.kl_I; }
        }
        off[j] = steps;                                   // the count, replaced by the offset below
        sum = min(sum + steps, sat);
    }
    const int incl = ed_scan(part, tid, sum, sat);
    const int total = part[kEdThreads - 1];
    // offsets saturate with the sums; they are read only when total <= cap_items, and then nothing saturated
    int run = incl - sum;
    for (int j = lo; j < hi; j++) {
        const int c = off[j];
        off[j] = run;
        run = min(run + c, sat);
    }
    if (tid == 0) {
        const bool over = total > a.cap_items;
        off[n] = over ? 0 : total;
        a.items[seq] = over ? 0 : total;
        if (over) atomicOr(a.status + seq, EDGEHIP_EDGEMAP_ITEM_OVERFLOW);
        else atomicAnd(a.status + seq, ~EDGEHIP_EDGEMAP_ITEM_OVERFLOW);
    }
}

}  // namespace edgehip

using namespace edgehip;

struct edgehip_ctx::EdgeMapDecode {
    int cap_segments = 0, cap_items = 0;
    std::vector<void *> dev;
    float *seg = nullptr;
    uint8_t *flag = nullptr;
    int32_t *seg_num = nullptr, *status = nullptr, *seg_off = nullptr, *items = nullptr, *cell = nullptr, *ids = nullptr, *s_num = nullptr;
    double *seg_dir = nullptr, *pose = nullptr;
    bool decoded = false;              // an edgehip_edgemap_decode was enqueued since the enable
    hipEvent_t ev_t[4][2] = {};        // around the last decode / hide / items / fill launch made under edgehip_profile_enable
    bool timed[4] = {false, false, false, false};
};

void edgehip::edgemap_decode_free(edgehip_ctx *c) {
    auto *d = c->emdec;
    if (!d) return;
    (void)hipStreamSynchronize(c->stream);
    for (void *q : d->dev) (void)hipFree(q);
    for (auto &pair : d->ev_t)
        for (hipEvent_t e : pair)
            if (e) (void)hipEventDestroy(e);
    delete d;
    c->emdec = nullptr;
}

template <class T> static bool ed_alloc(edgehip_ctx::EdgeMapDecode *d, T **p, size_t count) {
    void *q = nullptr;
    if (hipMalloc(&q, sizeof(T) * std::max<size_t>(count, 1)) != hipSuccess) { (void)hipGetLastError(); return false; }
    d->dev.push_back(q);
    *p = (T *)q;
    return true;
}

static em::SegCam ed_camera(const edgehip_ctx *c) {
    em::SegCam cam;
    cam.ppx = c->plan.ppx; cam.ppy = c->plan.ppy; cam.zfm = c->plan.zfm;
    cam.w = (uint32_t)c->plan.w; cam.h = (uint32_t)c->plan.h;
    return cam;
}

static EdArgs ed_args(edgehip_ctx *c) {
    auto *d = c->emdec;
    EdArgs a = {};
    a.seg = d->seg; a.flag = d->flag; a.seg_num = d->seg_num; a.status = d->status; a.seg_off = d->seg_off; a.seg_dir = d->seg_dir;
    a.items = d->items; a.pose = d->pose; a.s_num = d->s_num;
    a.cap_segments = d->cap_segments; a.cap_items = d->cap_items;
    a.cam = ed_camera(c);
    return a;
}

void edgehip::edgemap_decode_mark(edgehip_ctx *c, int stage, bool end) {
    auto *d = c->emdec;
    if (!end) d->timed[stage] = c->prof->on;
    if (d->timed[stage]) (void)hipEventRecord(d->ev_t[stage][end ? 1 : 0], c->stream);
}
struct EdTimer {   // HIP events around one launch when the profiler is on
    edgehip_ctx *c;
    int stage;
    EdTimer(edgehip_ctx *ctx, int st) : c(ctx), stage(st) { edgemap_decode_mark(c, stage, false); }
    ~EdTimer() { edgemap_decode_mark(c, stage, true); }
};

int edgehip_edgemap_decode_enable(edgehip_ctx *c, int cap_segments, int cap_items) {
    EH_ENTER(c);
    if (cap_segments < 0 || cap_items < 0 || cap_segments > (1 << 24) || cap_items > (1 << 24)) {
        set_error("edgemap_decode_enable: cap_segments and cap_items must be in [0, 2^24]");
        return EDGEHIP_ERR_ARG;
    }
    edgemap_decode_free(c);
    if (cap_segments == 0) return 0;
    auto *d = c->emdec = new edgehip_ctx::EdgeMapDecode;
    const size_t B = c->plan.nseq, S = cap_segments, I = cap_items;
    d->cap_segments = cap_segments;
    d->cap_items = cap_items;
    bool ok = ed_alloc(d, &d->seg, B * S * 8) && ed_alloc(d, &d->flag, B * S) && ed_alloc(d, &d->seg_num, B) && ed_alloc(d, &d->status, B) &&
              ed_alloc(d, &d->seg_off, B * (S + 1)) && ed_alloc(d, &d->seg_dir, B * S * 4) && ed_alloc(d, &d->items, B) &&
              ed_alloc(d, &d->cell, B * I) && ed_alloc(d, &d->ids, B * I) && ed_alloc(d, &d->s_num, B) && ed_alloc(d, &d->pose, B * 16);
    for (auto &pair : d->ev_t)
        for (hipEvent_t &e : pair) ok = ok && hipEventCreate(&e) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        edgemap_decode_free(c);
        set_error("edgemap_decode_enable: allocation failed");
        return EDGEHIP_ERR_MEMORY;
    }
    hipError_t z = hipMemsetAsync(d->seg_num, 0, sizeof(int32_t) * B, c->stream);
    if (z == hipSuccess) z = hipMemsetAsync(d->status, 0, sizeof(int32_t) * B, c->stream);
    if (z == hipSuccess) z = hipMemsetAsync(d->items, 0, sizeof(int32_t) * B, c->stream);
    if (z != hipSuccess) edgemap_decode_free(c);
    EH_CHECK(z);
    return 0;
}

int edgehip_edgemap_decode(edgehip_ctx *c, double x_scaling, double y_scaling) {
    EH_ENTER(c);
    auto *d = c->emdec;
    if (!d) { set_error("edgemap_decode: the decoder is not enabled (edgehip_edgemap_decode_enable)"); return EDGEHIP_ERR_STATE; }
    EdArgs a = ed_args(c);
    if (!edgemap_store(c, &a.rec, &a.count, &a.rho_scale, &a.cap_records)) { set_error("edgemap_decode: the record store is not enabled (edgehip_edgemap_enable)"); return EDGEHIP_ERR_STATE; }
    if (!(x_scaling >= 0) || !(y_scaling >= 0) || !std::isfinite(x_scaling) || !std::isfinite(y_scaling)) { set_error("edgemap_decode: the scalings must be finite and >= 0"); return EDGEHIP_ERR_ARG; }
    a.x_scaling = x_scaling == 0 ? 0.5 : x_scaling;
    a.y_scaling = y_scaling == 0 ? 1.0 : y_scaling;
    {
        EdTimer t(c, 0);
        hipLaunchKernelGGL(k_em_decode, dim3(c->plan.nseq), dim3(kEdThreads), 0, c->stream, a);
    }
    EH_LAUNCH_CHECK();
    d->decoded = true;
    return 0;
}

int edgehip_edgemap_hide_visible(edgehip_ctx *c, const double *const *dpose, const double *const *dpos, const float *k_em, const float *k_new,
                                 int32_t *s_num_out) {
    EH_ENTER(c);
    auto *d = c->emdec;
    if (!d) { set_error("edgemap_hide_visible: the decoder is not enabled (edgehip_edgemap_decode_enable)"); return EDGEHIP_ERR_STATE; }
    if (!d->decoded) { set_error("edgemap_hide_visible: nothing was decoded yet (edgehip_edgemap_decode)"); return EDGEHIP_ERR_STATE; }
    if (!dpose || !dpos || !k_em || !k_new) { set_error("edgemap_hide_visible: null argument"); return EDGEHIP_ERR_ARG; }
    const int B = c->plan.nseq;
    std::vector<double> pose((size_t)B * 16, 0.0);
    for (int s = 0; s < B; s++) {
        if (!dpose[s] || !dpos[s]) continue;
        double *P = pose.data() + (size_t)s * 16;
        for (int i = 0; i < 9; i++) P[i] = dpose[s][i];
        for (int i = 0; i < 3; i++) P[9 + i] = dpos[s][i];
        P[12] = k_em[s]; P[13] = k_new[s]; P[14] = 1;
    }
    EH_CHECK(hipMemcpyAsync(d->pose, pose.data(), sizeof(double) * pose.size(), hipMemcpyHostToDevice, c->stream));
    EH_CHECK(hipMemsetAsync(d->s_num, 0, sizeof(int32_t) * (size_t)B, c->stream));
    const EdArgs a = ed_args(c);
    {
        EdTimer t(c, 1);
        hipLaunchKernelGGL(k_em_hide, dim3((d->cap_segments + kEdThreads - 1) / kEdThreads, B), dim3(kEdThreads), 0, c->stream, a);
    }
    EH_LAUNCH_CHECK();
    if (s_num_out) EH_CHECK(hipMemcpyAsync(s_num_out, d->s_num, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, c->stream));
    EH_CHECK(hipStreamSynchronize(c->stream));   // the staged poses are the caller's until here
    if (s_num_out)
        for (int s = 0; s < B; s++)
            if (!dpose[s] || !dpos[s]) s_num_out[s] = -1;
    return 0;
}

int edgehip::edgemap_items_enqueue(edgehip_ctx *c, double v_thresh, double a_thresh_deg, int use_visibility, SegSource *out) {
    auto *d = c->emdec;
    if (!d) { set_error("depth_fill_segments: the decoder is not enabled (edgehip_edgemap_decode_enable)"); return EDGEHIP_ERR_STATE; }
    if (!d->decoded) { set_error("depth_fill_segments: nothing was decoded yet (edgehip_edgemap_decode)"); return EDGEHIP_ERR_STATE; }
    EdArgs a = ed_args(c);
    a.v_thresh = v_thresh;
    a.cos_a = std::cos(a_thresh_deg * M_PI / 180.0);
    a.use_visibility = use_visibility != 0;
    {
        EdTimer t(c, 2);
        hipLaunchKernelGGL(k_em_items, dim3(c->plan.nseq), dim3(kEdThreads), 0, c->stream, a);
    }
    EH_LAUNCH_CHECK();
    out->seg = d->seg; out->seg_num = d->seg_num; out->seg_off = d->seg_off; out->seg_dir = d->seg_dir; out->items = d->items;
    out->cell = d->cell; out->ids = d->ids; out->cap_segments = d->cap_segments; out->cap_items = d->cap_items;
    return 0;
}

int edgehip_download_edgemap_segments_batch(edgehip_ctx *c, int n, const int32_t *seqs, float *const *segments, uint8_t *const *flags,
                                            int32_t *counts, int32_t *status) {
    EH_ENTER(c);
    auto *d = c->emdec;
    if (!d) { set_error("download_edgemap_segments: the decoder is not enabled"); return EDGEHIP_ERR_STATE; }
    if (n < 1 || !seqs) { set_error("download_edgemap_segments: bad argument"); return EDGEHIP_ERR_ARG; }
    const int B = c->plan.nseq;
    for (int j = 0; j < n; j++)
        if (seqs[j] < 0 || seqs[j] >= B) { set_error("download_edgemap_segments: sequence out of range"); return EDGEHIP_ERR_ARG; }
    std::vector<int32_t> cs(2 * (size_t)B);
    EH_CHECK(hipMemcpyAsync(cs.data(), d->seg_num, sizeof(int32_t) * B, hipMemcpyDeviceToHost, c->stream));
    EH_CHECK(hipMemcpyAsync(cs.data() + B, d->status, sizeof(int32_t) * B, hipMemcpyDeviceToHost, c->stream));
    EH_CHECK(hipStreamSynchronize(c->stream));
    bool any = false;
    for (int j = 0; j < n; j++) {
        const int k = std::max(0, std::min(cs[seqs[j]], d->cap_segments));
        if (counts) counts[j] = k;
        if (status) status[j] = cs[B + seqs[j]];
        if (k == 0) continue;
        const size_t o = (size_t)seqs[j] * d->cap_segments;
        if (segments && segments[j]) { EH_CHECK(hipMemcpyAsync(segments[j], d->seg + o * 8, sizeof(float) * 8 * k, hipMemcpyDeviceToHost, c->stream)); any = true; }
        if (flags && flags[j]) { EH_CHECK(hipMemcpyAsync(flags[j], d->flag + o, (size_t)k, hipMemcpyDeviceToHost, c->stream)); any = true; }
    }
    if (any) EH_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int edgehip_download_edgemap_segments(edgehip_ctx *c, int seq, float *segments, uint8_t *flags, int32_t *count, int32_t *status) {
    return edgehip_download_edgemap_segments_batch(c, 1, &seq, &segments, &flags, count, status);
}

int edgehip_edgemap_decode_ms(edgehip_ctx *c, float ms[4]) {
    EH_ENTER(c);
    auto *d = c->emdec;
    if (!d || !ms) { set_error("edgemap_decode_ms: the decoder is not enabled, or null argument"); return EDGEHIP_ERR_STATE; }
    for (int i = 0; i < 4; i++) {
        ms[i] = -1.f;
        if (!d->timed[i]) continue;
        EH_CHECK(hipEventSynchronize(d->ev_t[i][1]));
        EH_CHECK(hipEventElapsedTime(ms + i, d->ev_t[i][0], d->ev_t[i][1]));
    }
    return 0;
}
