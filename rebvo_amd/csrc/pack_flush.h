// pack_flush.h — a workgroup's part of a packed record store, out of LDS (k_net_pack, k_ros_pack).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace edgehip {

// `img` is an LDS image of `nw` consecutive 16-byte words of `store`, laid out from the word at byte address w0 (a multiple of 16) on;
// of those words the workgroup owns the bytes [b0, b1).  The words that lie wholly inside [b0, b1) go out as 16-byte nontemporal
// stores.  The first and the last word of the range may be shared with the neighbouring workgroup or, at the ends of a sequence's
// list, hold bytes that are not the sequence's: of those only the workgroup's own bytes are written, in granules of type G (b0, b1 and
// every record are multiples of sizeof(G): uint8_t for the 15-byte net_keyline, uint32_t for the ROS records).  Nothing outside
// [b0, b1) is ever written, so neighbouring workgroups and neighbouring sequences never touch the same byte.  Call it with all T
// threads of the workgroup, behind the barrier that completes the image.
template <typename G, int T>
__device__ __forceinline__ void flush_words(const uint8_t *img, uint8_t *store, const size_t w0, const int nw, const size_t b0, const size_t b1) {
    typedef uint32_t u4v __attribute__((ext_vector_type(4)));
    for (int t = threadIdx.x; t < nw; t += T) {
        const size_t g = w0 + (size_t)t * 16;
        if (g >= b0 && g + 16 <= b1) {
            const u4v v = *reinterpret_cast<const u4v *>(img + t * 16);
            __builtin_nontemporal_store(v, reinterpret_cast<u4v *>(store + g));
        } else {   // partial (or, past either end of the range, not the workgroup's at all)
#pragma unroll
            for (int i = 0; i < 16; i += (int)sizeof(G))
                if (g + i >= b0 && g + i < b1) *reinterpret_cast<G *>(store + g + i) = *reinterpret_cast<const G *>(img + t * 16 + i);
        }
    }
}

}  // namespace edgehip
