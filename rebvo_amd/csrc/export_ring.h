// export_ring.h — the staging ring behind the output callbacks at full pipeline depth (edgehip_export_keylines, edgehip_ros_export).
//
// What a callback receives of frame k-1 is packed in-stream, right behind the frame that finishes with the slot, into one of R entries
// on the device; the slot is free again as far as callbacks go, the copies to the host run on a stream of the ring's own under the
// frames that follow, and nothing synchronises the frame streams.  The ring moves bytes: what an entry holds and what a request row
// says is its user's business (the packing kernel, the layout of an entry, the argument checks).  The functions are in api.hip.
//
// An entry belongs to its ticket from claim() to release().  The packing kernel reads the entry's request row in place and writes its
// device bytes, so release() lets go of a ticket that was never fetched only behind its pack event: the next ticket of that entry may
// ask for something else.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

struct edgehip_ctx;

namespace edgehip {

struct ExportRing {
    static constexpr int R = 4;       // tickets in flight (a group keeps at most three: two steps in flight + the one being delivered)
    hipStream_t stream = nullptr;     // the copies to the host (never the log's stream: edgehip_read_nav_log synchronises that one)
    hipEvent_t ev_pack[R] = {}, ev_done[R] = {};   // [entry] its packing kernel / its copies to the host have finished
    int n_cap = 0;                    // lists per entry the memory below has room for
    size_t entry_bytes = 0, row_bytes = 0;
    uint8_t *dev = nullptr;           // [R][entry_bytes]
    uint8_t *rows = nullptr;          // page-locked [R][row_bytes]: an entry's request, read in place by the packing kernel
    uint8_t *host[R] = {};            // page-locked [entry_bytes] mirror of an entry, allocated when a destination is not page-locked itself
    struct Copy { void *dst; size_t off, bytes; };   // bytes [off, off + bytes) of an entry, to the host
    struct Ticket { long long id = -1; int n = 0, what = 0; bool fetched = false; std::vector<Copy> staged; } t[R];
    long long next = 0;

    uint8_t *entry(int e) const { return dev + (size_t)e * entry_bytes; }
    uint8_t *row(int e) const { return rows + (size_t)e * row_bytes; }

    // `who` is the entry point's name in error messages.  Everything returns 0 or an EDGEHIP_ERR_* code.
    int open(bool highest_priority);   // the stream and the events, on first use
    // room for n lists per entry (grown by the caller's rule, never shrunk): only with no ticket outstanding.  Synchronises both streams;
    // the new entries are zeroed on c->stream; a failure leaves the ring without memory (n_cap == 0)
    int reserve(edgehip_ctx *c, const char *who, int n, size_t entry_bytes, size_t row_bytes);
    int claim(const char *who, int *e);   // the next entry, unless its ticket is still outstanding
    // behind the packing kernel's launch on c->stream: the entry's pack event, the slot's read-done event, the ticket
    int commit(edgehip_ctx *c, int e, int slot, int n, int what, int *ticket_out);
    Ticket *find(int ticket, int *e);
    // the copies of a ticket: straight into a destination inside a range of edgehip_register_host, through the entry's mirror and a
    // host copy in release() otherwise
    int fetch(const char *who, int e, const std::vector<Copy> &copies);
    int release(int e);                // block until the ticket's copies have landed (or, never fetched, its pack has run); frees the entry
    void drop_memory();                // back to n_cap == 0 (nothing may be in flight)
    void close();                      // edgehip_destroy
};

}  // namespace edgehip
