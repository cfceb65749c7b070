// keyframe_track.h — what keyframe_track.hip (the current key frame and its repair) and keyframe_list.hip (the ring of retired key
// frames) share: the per-sequence key-frame state, the list's device view, and the store behind edgehip_ctx::kftrack.
#pragma once
#include "ctx.h"

#include <vector>

namespace edgehip {

struct KfSeq {
    edgehip_kf_pose pose;
    int32_t kn, kf_count, active, do_insert;
    double Ef[9], Eb[9];     // forwardCorrectAugmentate's / correctAugmentate's E of the running frame
};

// ---- the key-frame list (keyframe_list.hip) ------------------------------------------------------------------------------------------
// Per sequence a ring of `capacity` entries; the key frame with ordinal j (the j-th the sequence ever took, from 0) lives in ring
// position j % capacity.  An entry is a header and room for max_points 168-byte records; headers and records are two arrays, so that
// every entry's records start at a multiple of 16 bytes (the stride is max_points * 168 rounded up to 16: an odd max_points alone
// would not give that).  Memory: (stride + 264 B) * capacity * nseq.
struct KfListHdr {
    edgehip_kf_pose pose;
    int32_t kn, ordinal;
};
struct KfListSeq {
    int32_t first, held, overwritten;   // the held ordinals are [first, first + held); entries lost to the ring so far
    int32_t retire_kn, retire_pos;      // of the retirement under way: KeyLines of the outgoing key frame (-1: none) and its ring position
    int32_t pad;
};
struct KfListDev {           // by value into the kernels; hdr == nullptr: the list is off
    uint8_t *rec;            // [nseq][capacity] entries of `stride` bytes
    KfListHdr *hdr;          // [nseq][capacity]
    KfListSeq *ls;           // [nseq]
    size_t stride;
    int capacity, cap;       // ring entries; max_points
};

// The outgoing key frame's header goes into the list and the sequence's retirement is posted for k_kf_retire.  Called by the one thread
// that is about to overwrite ks[seq] (k_kf_decide, k_kf_retire_mark), BEFORE it does: `k` is the outgoing state.
__device__ inline void kf_list_retire_head(const KfListDev &l, int seq, const KfSeq &k, bool retire) {
    KfListSeq &q = l.ls[seq];
    if (!retire || k.kf_count <= 0) { q.retire_kn = -1; return; }
    const int ordinal = k.kf_count - 1, pos = ordinal % l.capacity;
    KfListHdr &h = l.hdr[(size_t)seq * l.capacity + pos];
    h.pose = k.pose;
    h.kn = max(0, min(k.kn, l.cap));
    h.ordinal = ordinal;
    if (q.held == l.capacity) { q.first++; q.overwritten++; }
    else q.held++;
    q.retire_kn = h.kn;
    q.retire_pos = pos;
}

// ---- the positions of a sequence (keyframe_covis.hip, keyframe_reloc.hip) --------------------------------------------------------------
// Position t of a sequence: its held list entries, oldest first, then its current key frame; position M (= list capacity + 1) is the ring
// slot of the query forms.
struct CvKf {                // a position of a sequence: kn < 0: the sequence has no key frame there
    double Pose[9], Pos[3], K;
    int32_t kn, src;         // src >= 0: list ring position; -1: the current key frame; -2: the ring slot of the query form
};
static_assert(sizeof(CvKf) == 112, "13 doubles + 2 ints");

__device__ inline CvKf kf_position(const int seq, const int pos, const int M, const int cap, const KfSeq *__restrict__ ks, const KfListDev &l,
                                   const int32_t *__restrict__ slot_kn, const edgehip_kf_pose *__restrict__ pose_in, const SeqDev *__restrict__ seqs,
                                   const edgehip_nav *__restrict__ nav) {
    const int first = l.hdr ? l.ls[seq].first : 0, held = l.hdr ? max(0, min(l.ls[seq].held, l.capacity)) : 0;
    CvKf d;
    d.kn = -1; d.src = -1; d.K = 1.0;
    for (int i = 0; i < 9; i++) d.Pose[i] = 0.0;
    for (int i = 0; i < 3; i++) d.Pos[i] = 0.0;
    const edgehip_kf_pose *p = nullptr;
    if (pos < M && pos < held) {
        const int at = (first + pos) % l.capacity;
        const KfListHdr &h = l.hdr[(size_t)seq * l.capacity + at];
        d.kn = max(0, min(h.kn, cap)); d.src = at;
        p = &h.pose;
    } else if (pos < M && pos == held && ks[seq].kf_count > 0) {
        d.kn = max(0, min(ks[seq].kn, cap)); d.src = -1;
        p = &ks[seq].pose;
    } else if (pos == M && slot_kn) {
        d.kn = max(0, min(slot_kn[seq], cap)); d.src = -2;
        if (pose_in) p = &pose_in[seq];
        else {   // what edgehip_keyframe_insert takes by default: the newest nav record's pose and seq_state's K
            for (int i = 0; i < 9; i++) d.Pose[i] = nav[seq].Pose[i];
            for (int i = 0; i < 3; i++) d.Pos[i] = nav[seq].Pos[i];
            d.K = seqs[seq].pub.K;
        }
    }
    if (p) {
        for (int i = 0; i < 9; i++) d.Pose[i] = p->Pose[i];
        for (int i = 0; i < 3; i++) d.Pos[i] = p->Pos[i];
        d.K = p->K;
    }
    return d;
}

}  // namespace edgehip

struct edgehip_ctx::KfTrack {
    double save_percent = 0;
    int save_keyframes = 0;
    bool in_driver = true;            // edgehip_process_frame runs the steps (enable == 1); false: the store and the stage-level entry points alone
    int use_lds = 1;
    int np2cap = 1;
    std::vector<void *> dev;          // every device allocation
    std::vector<edgehip::KlSoA> kl;   // [nseq] host copies of the key frames' array pointers
    edgehip::KlSoA *kl_dev = nullptr; // [nseq]
    edgehip::KfSeq *ks = nullptr;     // [nseq]
    edgehip_kf_track *rec = nullptr;  // [nseq]
    int32_t *table = nullptr;         // [nseq][cap] buildForwardMatch's fowMatch
    double *dist = nullptr;           // [nseq][cap]
    uint32_t *keys = nullptr;         // [nseq][np2cap]
    edgehip_keyline *aos = nullptr;   // [cap] staging of upload / download
    // a caller's Pose / Pos, pose blocks and mask on their way to an in-stream kernel
    double *pose12_dev = nullptr, *pose12_host = nullptr;           // [nseq][12]
    edgehip_kf_pose *blk_dev = nullptr, *blk_host = nullptr;        // [nseq]
    uint8_t *mask_dev = nullptr, *mask_host = nullptr;              // [nseq]
    hipEvent_t ev = nullptr;
    bool busy = false;
    // the key-frame list (keyframe_list.hip); list.hdr == nullptr: off
    edgehip::KfListDev list = {};
    void *list_arena = nullptr;       // records | headers | per-sequence state | restore requests
    int32_t *list_req_dev = nullptr, *list_req_host = nullptr;      // [nseq] edgehip_keyframe_list_restore's ring positions
    // keyframe_covis.hip's scratch: allocated by the first call, for covis_m = list capacity + 1 positions per sequence
    void *covis_arena = nullptr;
    int covis_m = 0;
    double covis_ms[2] = {0, 0};      // the last call's device time: field build (with the gather), pair pass
    // keyframe_reloc.hip's scratch: allocated by the first edgehip_keyframe_relocalize, for reloc_m = list capacity + 1 positions per sequence
    void *reloc_arena = nullptr;
    int reloc_m = 0;
    double reloc_ms[2] = {0, 0};      // the last call's device time: prepare (gather, set-up, fields), solve
    // keyframe_constraint.hip's scratch: the rows, allocated by the first edgehip_keyframe_constraint (92 B per KeyLine of capacity and sequence)
    void *kc_arena = nullptr;
    int32_t *kc_counts = nullptr;     // [nseq][2] edgehip_keyframe_mutual_exclusion's (links seen, links kept); allocated with the key frames
    double kc_ms[2] = {0, 0};         // the last constraint call's device time: gather, solve
    // keyframe_depth.hip's scratch, allocated by the first of its calls: the caller's poses on their way in ([nseq][13], device row and
    // page-locked row), the results ([nseq]); events: the last call's begin and end, the last copy out of the page-locked row
    double *kd_pose_dev = nullptr, *kd_pose_host = nullptr;
    edgehip_kf_depth *kd_out_dev = nullptr;
    hipEvent_t kd_ev[3] = {nullptr, nullptr, nullptr};
    uint8_t *kd_mask_dev = nullptr;   // [nseq] edgehip_keyframe_depth_select's mask (read while kd_masked)
    bool kd_busy = false, kd_timed = false, kd_masked = false;
};

namespace edgehip {

void kf_list_free(edgehip_ctx *c);                   // behind a synchronisation of c->stream; no-op when off
int kf_list_reset_enqueue(edgehip_ctx *c);           // edgehip_reset: no entries (no-op when off)
// Behind a k_kf_decide that was given the list: the records of the posted retirements, before k_kf_copy overwrites them (no-op when off).
int kf_list_retire_enqueue(edgehip_ctx *c);
// edgehip_upload_keyframe: posts the retirement of sequence `seq`'s key frame (if it has one) and enqueues its records (no-op when off).
int kf_list_retire_one_enqueue(edgehip_ctx *c, int seq);
// What every stage-level entry point that reads ring slot `slot` does first: EDGEHIP_ERR_STATE without key-frame tracking, EDGEHIP_ERR_ARG
// for a slot out of range, then the slot's KeyLines as edgehip_download_keylines returns them, ordered behind stage A.
int kf_entry(edgehip_ctx *c, int slot, const char *who);
void kf_covis_free(edgehip_ctx *c);                  // keyframe_covis.hip's scratch; behind a synchronisation of c->stream; no-op when absent
void kf_reloc_free(edgehip_ctx *c);                  // keyframe_reloc.hip's scratch; the same
void kf_constraint_free(edgehip_ctx *c);             // keyframe_constraint.hip's scratch; the same
void kf_depth_free(edgehip_ctx *c);                  // keyframe_depth.hip's scratch; the same

}  // namespace edgehip
