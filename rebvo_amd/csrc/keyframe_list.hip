// keyframe_list.hip — the reference's REBVO::kf_list (rebvo.h:437, rebvo_second_t.cpp:156-162, 591-596) for whole batches: every key
// frame a sequence replaces is kept, in HBM, as the 168-byte KeyLine records keyframe::dumpToBinaryFile writes (keyframe.cpp:73-147,
// edge_finder.cpp:411-419), in the state it had when it was replaced — its m_id_f after the last repair.  keyframe_track.hip holds only
// kf_list.back(); this file holds the rest, in a ring per sequence (keyframe_track.h has the layout).
//
// Retiring is in-stream and predicated like k_kf_copy: the single thread of k_kf_decide that is about to overwrite a sequence's pose
// block, kn and count writes the outgoing header into the ring first and posts (kn, ring position); k_kf_retire, launched between
// k_kf_decide and k_kf_copy over the whole batch, turns the 21 (24 with stereo) SoA arrays of the outgoing key frame into records.
// Sequences that retire nothing leave at once, so a frame that inserts nothing pays one launch of empty workgroups per hook.
//
// The store: a workgroup owns kKlTile = 256 consecutive records = 43008 B = 2688 whole 16-byte words (entry bases are multiples of 16),
// lane j reads KeyLine j of every array (coalesced), builds the record in registers, puts it at its byte position in an LDS image of
// the tile (8-byte LDS stores: a record is 21 of them), and flush_words (pack_flush.h) writes the image out as 16-byte nontemporal
// stores.  kn * 168 is a multiple of 16 only for even kn: the last word of an odd list is half the list's and goes out as one 8-byte
// store; the 8 bytes behind it are not written.
//
// Restoring is the way back: the tile's words come in as coalesced 16-byte loads into LDS, lane j takes record j apart into the ring
// slot's SoA arrays, MatchRec and gather record included, as edgehip_upload_keylines does on the host.
#include "keyframe_track.h"
#include "pack_flush.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace edgehip {

constexpr int kKlTile = 256;                      // records (and threads) per workgroup
constexpr int kKlBytes = (int)sizeof(edgehip_keyline);
static_assert(kKlBytes == 168, "the reference's KeyLine is 168 bytes");
static_assert((kKlTile * kKlBytes) % 16 == 0, "a tile is a whole number of 16-byte words");
static_assert(offsetof(edgehip_keyline, score) == 24 && offsetof(edgehip_keyline, c_p) == 28 && offsetof(edgehip_keyline, rho) == 40 &&
              offsetof(edgehip_keyline, p_m) == 88 && offsetof(edgehip_keyline, m_id) == 104 && offsetof(edgehip_keyline, m_m0) == 120 &&
              offsetof(edgehip_keyline, n_m0) == 128 && offsetof(edgehip_keyline, p_id) == 136 && offsetof(edgehip_keyline, stereo_rho) == 152,
              "edgehip_keyline is the reference's KeyLine byte for byte");
static_assert(sizeof(KfListHdr) == 264, "pose block (32 doubles) + kn + ordinal");

union KlWords {              // a record as the 21 8-byte words it is stored as; zeroed first, so that bytes 36..39 are zero
    edgehip_keyline o;
    uint64_t q[kKlBytes / 8];
};

// edgehip_upload_keyframe's retirement: sequence `only` alone (k_kf_decide does this for the other three places)
__global__ void k_kf_retire_mark(const KfSeq *__restrict__ ks, KfListDev l, int only, int nseq) {
    const int seq = blockIdx.x * blockDim.x + threadIdx.x;
    if (seq >= nseq) return;
    kf_list_retire_head(l, seq, ks[seq], seq == only);
}

__global__ __launch_bounds__(kKlTile) void k_kf_retire(const KlSoA *__restrict__ kf_kl, KfListDev l) {
    __shared__ __align__(16) uint8_t img[kKlTile * kKlBytes];
    const int seq = blockIdx.y, tid = threadIdx.x;
    const int kn = min(l.ls[seq].retire_kn, l.cap), r0 = blockIdx.x * kKlTile;
    if (kn <= r0) return;                     // block-uniform: nothing retires (-1), or the list ends before this tile
    const int i = r0 + tid;
    if (i < kn) {
        const KlSoA &k = kf_kl[seq];
        KlWords u;
#pragma unroll
        for (int w = 0; w < kKlBytes / 8; w++) u.q[w] = 0;
        edgehip_keyline &o = u.o;
        o.p_inx = k.p_inx[i];
        const float2 m_m = k.m_m[i], u_m = k.u_m[i], c_p = k.c_p[i], p_m = k.p_m[i], p_m_0 = k.p_m_0[i], m_m0 = k.m_m0[i];
        o.m_m[0] = m_m.x; o.m_m[1] = m_m.y; o.u_m[0] = u_m.x; o.u_m[1] = u_m.y;
        o.n_m = k.n_m[i]; o.score = 0.f;
        o.c_p[0] = c_p.x; o.c_p[1] = c_p.y;
        o.rho = k.rho[i]; o.s_rho = k.s_rho[i]; o.rho_nr = k.rho_nr[i]; o.s_rho_nr = k.s_rho_nr[i]; o.rho0 = k.rho0[i]; o.s_rho0 = k.s_rho0[i];
        o.p_m[0] = p_m.x; o.p_m[1] = p_m.y; o.p_m_0[0] = p_m_0.x; o.p_m_0[1] = p_m_0.y;
        o.m_id = k.m_id[i]; o.m_id_f = k.m_id_f[i]; o.m_id_kf = k.m_id_kf[i]; o.m_num = k.m_num[i];
        o.m_m0[0] = m_m0.x; o.m_m0[1] = m_m0.y; o.n_m0 = k.n_m0[i];
        o.p_id = k.p_id[i]; o.n_id = k.n_id[i];
        o.net_id = -1; o.stereo_m_id = -1; o.stereo_rho = 1.0; o.stereo_s_rho = 20.0;   // what edgehip_download_keyframe gives the fields the device does not keep
        if (k.stereo_m_id) { o.stereo_m_id = k.stereo_m_id[i]; o.stereo_rho = k.stereo_rho[i]; o.stereo_s_rho = k.stereo_s_rho[i]; }
        uint64_t *dst = reinterpret_cast<uint64_t *>(img + tid * kKlBytes);
#pragma unroll
        for (int w = 0; w < kKlBytes / 8; w++) dst[w] = u.q[w];
    }
    __syncthreads();
    // the tile's bytes [b0, b1) of the entry; b1 <= max_points * 168 <= stride: nothing leaves the entry
    uint8_t *entry = l.rec + ((size_t)seq * l.capacity + l.ls[seq].retire_pos) * l.stride;
    const size_t b0 = (size_t)r0 * kKlBytes, b1 = (size_t)min(kn, r0 + kKlTile) * kKlBytes;
    flush_words<uint64_t, kKlTile>(img, entry, b0, (int)((b1 - b0 + 15) / 16), b0, b1);
}

// pos[seq]: the ring position to restore into the slot, or -1
__global__ __launch_bounds__(kKlTile) void k_kf_restore(const KlSoA *__restrict__ slot_kl, int32_t *__restrict__ slot_kn, float *__restrict__ slot_retuned,
                                                        KfListDev l, const int32_t *__restrict__ pos) {
    typedef uint32_t u4v __attribute__((ext_vector_type(4)));
    __shared__ __align__(16) uint8_t img[kKlTile * kKlBytes];
    const int seq = blockIdx.y, tid = threadIdx.x;
    const int at = pos[seq];
    if (at < 0 || at >= l.capacity) return;   // block-uniform
    const int kn = max(0, min(l.hdr[(size_t)seq * l.capacity + at].kn, l.cap)), r0 = blockIdx.x * kKlTile;
    if (blockIdx.x == 0 && tid == 0) { slot_kn[seq] = kn; slot_retuned[seq] = 0.f; }
    if (kn <= r0) return;
    // the words that hold the tile's records: the last one may reach 8 bytes past an odd list's end, still inside the entry (the stride
    // is a multiple of 16), and nothing reads those bytes out of the image
    const uint8_t *entry = l.rec + ((size_t)seq * l.capacity + at) * l.stride;
    const size_t b0 = (size_t)r0 * kKlBytes, b1 = (size_t)min(kn, r0 + kKlTile) * kKlBytes;
    const int nw = (int)((b1 - b0 + 15) / 16);
    for (int t = tid; t < nw; t += kKlTile)
        *reinterpret_cast<u4v *>(img + t * 16) = __builtin_nontemporal_load(reinterpret_cast<const u4v *>(entry + b0 + (size_t)t * 16));
    __syncthreads();
    const int i = r0 + tid;
    if (i >= kn) return;
    KlWords u;
    const uint64_t *src = reinterpret_cast<const uint64_t *>(img + tid * kKlBytes);
#pragma unroll
    for (int w = 0; w < kKlBytes / 8; w++) u.q[w] = src[w];
    const edgehip_keyline &o = u.o;
    const KlSoA &k = slot_kl[seq];
    k.p_inx[i] = o.p_inx;
    k.m_m[i] = make_float2(o.m_m[0], o.m_m[1]); k.u_m[i] = make_float2(o.u_m[0], o.u_m[1]); k.c_p[i] = make_float2(o.c_p[0], o.c_p[1]);
    k.p_m[i] = make_float2(o.p_m[0], o.p_m[1]); k.p_m_0[i] = make_float2(o.p_m_0[0], o.p_m_0[1]); k.m_m0[i] = make_float2(o.m_m0[0], o.m_m0[1]);
    k.n_m[i] = o.n_m;
    k.rho[i] = o.rho; k.s_rho[i] = o.s_rho; k.rho_nr[i] = o.rho_nr; k.s_rho_nr[i] = o.s_rho_nr; k.rho0[i] = o.rho0; k.s_rho0[i] = o.s_rho0;
    k.n_m0[i] = o.n_m0;
    k.m_id[i] = o.m_id; k.m_id_f[i] = o.m_id_f; k.m_id_kf[i] = o.m_id_kf; k.m_num[i] = o.m_num; k.p_id[i] = o.p_id; k.n_id[i] = o.n_id;
    MatchRec r;
    r.c_px = o.c_p[0]; r.c_py = o.c_p[1]; r.u_mx = o.u_m[0]; r.u_my = o.u_m[1]; r.m_mx = o.m_m[0]; r.m_my = o.m_m[1]; r.n_m = o.n_m; r.pad = 0.f;
    k.rec[i] = r;
    k.grec[i] = make_float4(o.c_p[0], o.c_p[1], o.m_m[0], o.m_m[1]);
    if (k.stereo_m_id) { k.stereo_m_id[i] = o.stereo_m_id; k.stereo_rho[i] = o.stereo_rho; k.stereo_s_rho[i] = o.stereo_s_rho; }
}

// a list switched on beside key frames that exist already starts with the current one's ordinal
__global__ void k_kf_list_init(const KfSeq *__restrict__ ks, KfListDev l, int nseq) {
    const int seq = blockIdx.x * blockDim.x + threadIdx.x;
    if (seq >= nseq) return;
    KfListSeq q = {};
    q.first = max(0, ks[seq].kf_count - 1);
    q.retire_kn = -1;
    l.ls[seq] = q;
}

}  // namespace edgehip

using namespace edgehip;

static dim3 kl_grid(edgehip_ctx *c) { return dim3((c->plan.cap + kKlTile - 1) / kKlTile, c->plan.nseq); }

void edgehip::kf_list_free(edgehip_ctx *c) {
    auto *d = c->kftrack;
    if (!d || !d->list.hdr) return;
    if (d->list_arena) (void)hipFree(d->list_arena);
    if (d->list_req_host) (void)hipHostFree(d->list_req_host);
    d->list = KfListDev();
    d->list_arena = nullptr; d->list_req_dev = nullptr; d->list_req_host = nullptr;
}

int edgehip::kf_list_reset_enqueue(edgehip_ctx *c) {
    auto *d = c->kftrack;
    if (!d || !d->list.hdr) return 0;
    // (behind the memset of the key frames' state: every count is 0, so every list starts at ordinal 0)
    hipLaunchKernelGGL(k_kf_list_init, dim3((c->plan.nseq + 63) / 64), dim3(64), 0, c->stream, (const KfSeq *)d->ks, d->list, c->plan.nseq);
    EH_LAUNCH_CHECK();
    return 0;
}

int edgehip::kf_list_retire_enqueue(edgehip_ctx *c) {
    auto *d = c->kftrack;
    if (!d->list.hdr) return 0;
    hipLaunchKernelGGL(k_kf_retire, kl_grid(c), dim3(kKlTile), 0, c->stream, (const KlSoA *)d->kl_dev, d->list);
    EH_LAUNCH_CHECK();
    return 0;
}

int edgehip::kf_list_retire_one_enqueue(edgehip_ctx *c, int seq) {
    auto *d = c->kftrack;
    if (!d->list.hdr) return 0;
    hipLaunchKernelGGL(k_kf_retire_mark, dim3((c->plan.nseq + 63) / 64), dim3(64), 0, c->stream, (const KfSeq *)d->ks, d->list, seq, c->plan.nseq);
    EH_LAUNCH_CHECK();
    return kf_list_retire_enqueue(c);
}

static int kl_entry(edgehip_ctx *c, const char *who, bool need_list) {
    if (!c->kftrack) { set_error(std::string(who) + ": key-frame tracking is not enabled (edgehip_keyframe_track_enable)"); return EDGEHIP_ERR_STATE; }
    if (need_list && !c->kftrack->list.hdr) { set_error(std::string(who) + ": the key-frame list is not enabled (edgehip_keyframe_list_enable)"); return EDGEHIP_ERR_STATE; }
    return 0;
}

int edgehip_keyframe_list_enable(edgehip_ctx *c, int capacity) {
    EH_ENTER(c);
    if (capacity < 0) { set_error("keyframe_list_enable: capacity must be >= 0"); return EDGEHIP_ERR_ARG; }
    if (!c->kftrack) {
        if (capacity == 0) return 0;
        return kl_entry(c, "keyframe_list_enable", false);
    }
    auto *d = c->kftrack;
    drop_frame_graphs(c);   // a captured frame holds the retire launches and the list's pointers, or neither
    EH_CHECK(hipStreamSynchronize(c->stream));
    kf_list_free(c);
    if (!capacity) return 0;
    const size_t B = c->plan.nseq, CAP = c->plan.cap;
    const size_t stride = (CAP * sizeof(edgehip_keyline) + 15) & ~(size_t)15;
    const size_t rec_bytes = B * (size_t)capacity * stride;                                  // a multiple of 16
    const size_t hdr_bytes = B * (size_t)capacity * sizeof(KfListHdr);                       // 264 B each: a multiple of 8
    const size_t ls_bytes = (B * sizeof(KfListSeq) + 15) & ~(size_t)15, req_bytes = B * sizeof(int32_t);
    void *arena = nullptr;
    bool ok = hipMalloc(&arena, rec_bytes + hdr_bytes + ls_bytes + req_bytes) == hipSuccess;
    ok = ok && hipHostMalloc((void **)&d->list_req_host, req_bytes, hipHostMallocDefault) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        if (arena) (void)hipFree(arena);
        if (d->list_req_host) (void)hipHostFree(d->list_req_host);
        d->list_req_host = nullptr;
        set_error("keyframe_list_enable: allocation failed (168 B x max_points x capacity x nseq)");
        return EDGEHIP_ERR_MEMORY;
    }
    d->list_arena = arena;
    KfListDev l;
    l.rec = (uint8_t *)arena;
    l.hdr = (KfListHdr *)(l.rec + rec_bytes);
    l.ls = (KfListSeq *)(l.rec + rec_bytes + hdr_bytes);
    d->list_req_dev = (int32_t *)(l.rec + rec_bytes + hdr_bytes + ls_bytes);
    l.stride = stride;
    l.capacity = capacity;
    l.cap = (int)CAP;
    d->list = l;
    // headers zeroed; the records are not (2.75 GB per unit of capacity at 1024 x 16000): only the kn records a retirement wrote are ever
    // handed out, padding included, and those it writes whole
    hipError_t e = hipMemsetAsync(l.hdr, 0, hdr_bytes, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_kf_list_init, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, c->stream, (const KfSeq *)d->ks, l, (int)B);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) kf_list_free(c);
    EH_CHECK(e);
    return 0;
}

int edgehip_keyframe_set_save(edgehip_ctx *c, int save_keyframes) {
    EH_ENTER(c);
    if (int e = kl_entry(c, "keyframe_set_save", false)) return e;
    const int v = save_keyframes != 0;
    if (v == c->kftrack->save_keyframes) return 0;
    drop_frame_graphs(c);   // the flag is a kernel argument of the captured frames
    c->kftrack->save_keyframes = v;
    return 0;
}

// ls[nseq] and the key frames' counts.  Synchronises.
static int kl_read_state(edgehip_ctx *c, std::vector<KfListSeq> &ls, std::vector<int32_t> &counts) {
    auto *d = c->kftrack;
    const size_t B = c->plan.nseq;
    std::vector<KfSeq> ks(B);
    ls.resize(B); counts.resize(B);
    EH_CHECK(hipMemcpyAsync(ls.data(), d->list.ls, sizeof(KfListSeq) * B, hipMemcpyDeviceToHost, c->stream));
    EH_CHECK(hipMemcpyAsync(ks.data(), d->ks, sizeof(KfSeq) * B, hipMemcpyDeviceToHost, c->stream));
    EH_CHECK(hipStreamSynchronize(c->stream));
    for (size_t s = 0; s < B; s++) counts[s] = ks[s].kf_count;
    return 0;
}

int edgehip_keyframe_list_info(edgehip_ctx *c, edgehip_kf_list_info *info) {
    EH_ENTER(c);
    if (int e = kl_entry(c, "keyframe_list_info", true)) return e;
    if (!info) return EDGEHIP_ERR_ARG;
    std::vector<KfListSeq> ls;
    std::vector<int32_t> counts;
    if (int e = kl_read_state(c, ls, counts)) return e;
    for (size_t s = 0; s < ls.size(); s++) {
        info[s].kf_count = counts[s];
        info[s].first = ls[s].first; info[s].held = ls[s].held; info[s].overwritten = ls[s].overwritten;
    }
    return 0;
}

static bool kl_held(const KfListSeq &q, int ordinal) { return ordinal >= q.first && ordinal < q.first + q.held; }

int edgehip_download_keyframe_list_batch(edgehip_ctx *c, int n, const int32_t *seqs, const int32_t *ordinals, edgehip_keyline *const *kl,
                                         int32_t *kn_out, edgehip_kf_pose *pose) {
    EH_ENTER(c);
    if (int e = kl_entry(c, "download_keyframe_list", true)) return e;
    if (n < 1 || !seqs || !ordinals) { set_error("download_keyframe_list: bad argument"); return EDGEHIP_ERR_ARG; }
    for (int j = 0; j < n; j++)
        if (seqs[j] < 0 || seqs[j] >= c->plan.nseq) { set_error("download_keyframe_list: sequence out of range"); return EDGEHIP_ERR_ARG; }
    auto *d = c->kftrack;
    const KfListDev &l = d->list;
    // one synchronisation for the lists' state and the requested headers' owners, one for the records
    std::vector<KfListSeq> ls;
    std::vector<int32_t> counts;
    std::vector<KfListHdr> hdr((size_t)c->plan.nseq * l.capacity);
    EH_CHECK(hipMemcpyAsync(hdr.data(), l.hdr, sizeof(KfListHdr) * hdr.size(), hipMemcpyDeviceToHost, c->stream));
    if (int e = kl_read_state(c, ls, counts)) return e;
    for (int j = 0; j < n; j++)
        if (!kl_held(ls[seqs[j]], ordinals[j])) { set_error("download_keyframe_list: the list does not hold that ordinal (overwritten, or not retired yet)"); return EDGEHIP_ERR_ARG; }
    for (int j = 0; j < n; j++) {
        const int pos = ordinals[j] % l.capacity;
        const KfListHdr &h = hdr[(size_t)seqs[j] * l.capacity + pos];
        if (kl && kl[j] && h.kn > 0)
            EH_CHECK(hipMemcpyAsync(kl[j], l.rec + ((size_t)seqs[j] * l.capacity + pos) * l.stride, sizeof(edgehip_keyline) * (size_t)h.kn,
                                    hipMemcpyDeviceToHost, c->stream));
        if (kn_out) kn_out[j] = h.kn;
        if (pose) pose[j] = h.pose;
    }
    EH_CHECK(hipStreamSynchronize(c->stream));
    return 0;
}

int edgehip_download_keyframe_list(edgehip_ctx *c, int seq, int ordinal, edgehip_keyline *kl, int32_t *kn_out, edgehip_kf_pose *pose) {
    const int32_t s = seq, o = ordinal;
    edgehip_keyline *const dst = kl;
    return edgehip_download_keyframe_list_batch(c, 1, &s, &o, &dst, kn_out, pose);
}

int edgehip_keyframe_list_restore(edgehip_ctx *c, int slot, const int32_t *ordinals) {
    EH_ENTER(c);
    if (int e = kl_entry(c, "keyframe_list_restore", true)) return e;
    if (slot < 0 || slot >= c->plan.nslots) { set_error("keyframe_list_restore: slot out of range"); return EDGEHIP_ERR_ARG; }
    if (!ordinals) { set_error("keyframe_list_restore: null ordinals"); return EDGEHIP_ERR_ARG; }
    auto *d = c->kftrack;
    std::vector<KfListSeq> ls;
    std::vector<int32_t> counts;
    if (int e = kl_read_state(c, ls, counts)) return e;
    const int B = c->plan.nseq;
    bool any = false;
    for (int s = 0; s < B; s++) {
        if (ordinals[s] == -1) continue;
        if (!kl_held(ls[s], ordinals[s])) { set_error("keyframe_list_restore: the list does not hold that ordinal (overwritten, or not retired yet)"); return EDGEHIP_ERR_ARG; }
        any = true;
    }
    if (!any) return 0;
    if (int e = rot_materialize_enqueue(c, slot)) return e;   // the other sequences of the slot keep their (turned) KeyLines
    if (int e = sync_all(c)) return e;                        // the slot's producers and readers on every stream; the request row is free
    for (int s = 0; s < B; s++) d->list_req_host[s] = ordinals[s] == -1 ? -1 : ordinals[s] % d->list.capacity;
    EH_CHECK(hipMemcpyAsync(d->list_req_dev, d->list_req_host, sizeof(int32_t) * B, hipMemcpyHostToDevice, c->stream));
    // The gather records are written, but whether u_m == m_m / |m_m| holds for what was restored is not known without reading it: the
    // slot goes back to the variant that fetches u_m (same results; edgehip_upload_keylines can afford the check, it has the records).
    if (c->grec_ok[slot]) { c->grec_ok[slot] = false; drop_frame_graphs(c); }
    hipLaunchKernelGGL(k_kf_restore, kl_grid(c), dim3(kKlTile), 0, c->stream, (const KlSoA *)kldev(c, slot), c->kn_slot + (size_t)slot * B,
                       c->retuned_slot + (size_t)slot * B, d->list, (const int32_t *)d->list_req_dev);
    EH_LAUNCH_CHECK();
    if (int e = order_a_after_bc(c)) return e;                // a stage-level call on the stage-A stream sees the restored slot
    return 0;
}
