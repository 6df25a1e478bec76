// Lock-free union-find on int32 parents for one-thread-per-point launches (lrg_baselines.hip, lrg_edge.hip).  The larger root is
// linked under the smaller, so a component's root is its minimum index whatever the order of the unions.  Visibility: the header
// comment of lrg_baselines.hip.
#pragma once
#include "lrg_common.h"

__device__ __forceinline__ int bl_load(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x with path halving (x's parent replaced by its grandparent by CAS: still an ancestor, still smaller)
__device__ __forceinline__ int bl_find(int32_t *parent, int x) {
    int p = bl_load(parent + x);
    while (p != x) {
        const int g = bl_load(parent + p);
        if (g == p) return p;
        int expect = p;
        __hip_atomic_compare_exchange_strong(parent + x, &expect, g, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = g;
    }
    return x;
}

__device__ __forceinline__ void bl_union(int32_t *parent, int x, int y) {
    int rx = bl_find(parent, x), ry = bl_find(parent, y);
    while (rx != ry) {
        const int hi = rx > ry ? rx : ry, lo = rx > ry ? ry : rx;
        int seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return;
        // hi was linked meanwhile: continue from the parent the CAS returned, not from a fresh load of parent[hi]
        rx = bl_find(parent, seen);
        ry = bl_find(parent, lo);
    }
}
