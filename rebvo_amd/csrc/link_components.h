// link_components.h — connected components of a KeyLine link graph and the sort of (component, index) keys, for the passes that run one
// lane per component (k_kf_augment's phase 2 in keyframe_track.hip is the form these were taken from; k_em_components in
// edgemap_compress.hip calls them).  One workgroup of T threads per list; `buf` holds one uint32 per KeyLine, in LDS or in HBM.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace edgehip {

__device__ __forceinline__ uint32_t lc_find(const uint32_t *lab, uint32_t i) {
    while (1) {
        const uint32_t l = __atomic_load_n(lab + i, __ATOMIC_RELAXED);
        if (l == i) return i;
        i = l;   // (a label only ever decreases and names a member of the same component: the chain ends at a root)
    }
}

// buf[i] <- the minimum index of i's component in the undirected graph of the links link(i, side), side < SIDES (a link outside [0, kn)
// or to i itself is no edge).  Atomic-min hooking + pointer jumping: the links need not be mutual, several KeyLines may share a
// successor, cycles and self-links occur — any link graph is handled.  `changed` is one int of LDS.  Ends behind a barrier.
template <int T, int SIDES, class Link>
__device__ __forceinline__ void lc_label_min(uint32_t *buf, const int kn, int *changed, Link link) {
    const int tid = threadIdx.x;
    for (int i = tid; i < kn; i += T) buf[i] = (uint32_t)i;
    __syncthreads();
    while (1) {
        if (tid == 0) *changed = 0;
        __syncthreads();
        for (int i = tid; i < kn; i += T) {
            for (int side = 0; side < SIDES; side++) {
                const int j = link(i, side);
                if (j < 0 || j >= kn || j == i) continue;
                const uint32_t ra = lc_find(buf, (uint32_t)i), rb = lc_find(buf, (uint32_t)j);
                if (ra != rb) {
                    atomicMin(buf + max(ra, rb), min(ra, rb));
                    *changed = 1;
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < kn; i += T) {
            const uint32_t r = lc_find(buf, (uint32_t)i);
            __atomic_store_n(buf + i, r, __ATOMIC_RELAXED);
        }
        const int again = *changed;
        __syncthreads();
        if (!again) break;
    }
}

// ascending bitonic sort of buf[0 .. np2), np2 a power of two.  Ends behind a barrier.
template <int T>
__device__ __forceinline__ void lc_sort(uint32_t *buf, const int np2) {
    const int tid = threadIdx.x;
    for (int size = 2; size <= np2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (np2 >> 1); t += T) {
                const int lo = ((t & ~(stride - 1)) << 1) | (t & (stride - 1)), hi = lo | stride;
                const uint32_t x = buf[lo], y = buf[hi];
                const bool up = (lo & size) == 0;
                if ((x > y) == up) { buf[lo] = y; buf[hi] = x; }
            }
            __syncthreads();
        }
}

}  // namespace edgehip
