// The voxel hash of a batch of rooms (lrg_baselines.hip, lrg_edge.hip): one linear-probe segment per room inside two arrays of
// 4 n + 64 n_rooms slots, so that a lookup never leaves its room.  Room r owns points room_start[r] .. room_start[r + 1] - 1; its
// segment starts at slot 4 room_start[r] + 64 r and has the smallest power of two >= max(64, 2 n_room) slots (< 4 n_room + 64).
#pragma once
#include "lrg_common.h"

// Bounds of room r (room_start was checked on the host: this only keeps a bad word from turning into an address)
__device__ __forceinline__ bool lrg_room_bounds(const int32_t *room_start, int n, int r, int *s, int *e) {
    const int s0 = room_start[r], e0 = room_start[r + 1];
    if (s0 < 0 || e0 < s0 || e0 > n) return false;
    *s = s0; *e = e0;
    return true;
}

__device__ __forceinline__ void lrg_room_segment(uint64_t *keys, int32_t *vals, int r, int s, int e, uint64_t **seg_keys, int32_t **seg_vals,
                                                 int *mask) {
    int cap = 64;
    while (cap < 2 * (e - s)) cap <<= 1;
    const long off = 4L * s + 64L * r;
    *seg_keys = keys + off; *seg_vals = vals + off; *mask = cap - 1;
}

// the last r with room_start[r] <= i (empty rooms are skipped)
__device__ __forceinline__ int lrg_room_of(const int32_t *room_start, int n_rooms, int i) {
    int lo = 0, hi = n_rooms - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (room_start[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// key -> i in the room's segment; false when the key is there already (two points of the room in one voxel)
__device__ __forceinline__ bool lrg_room_insert(uint64_t *keys, int32_t *vals, int mask, uint64_t key, int i) {
    unsigned h = (unsigned)lrg_fmix64(key) & (unsigned)mask;
    for (int probe = 0; probe <= mask; ++probe) {
        const unsigned long long prev = atomicCAS(reinterpret_cast<unsigned long long *>(&keys[h]), (unsigned long long)LRG_HASH_EMPTY,
                                                  (unsigned long long)key);
        if (prev == LRG_HASH_EMPTY) { vals[h] = i; return true; }
        if (prev == key) return false;
        h = (h + 1) & (unsigned)mask;
    }
    return true;
}
