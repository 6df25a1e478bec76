// The voxel hash of a batch of rooms (baselines, edge, FPFH, MCPNet, preprocessing): one linear-probe segment per room inside arrays of
// 4 n + 64 n_rooms slots, so that a lookup never leaves its room.  Room r owns points room_start[r] .. room_start[r + 1] - 1; its
// segment starts at slot 4 room_start[r] + 64 r and has the smallest power of two >= max(64, 2 n_room) slots (< 4 n_room + 64).
// This file is the only one that knows the rule; what a module does about a bad room or a key met twice is the module's own.
#pragma once
#include "lrg_common.h"

// slots of a batch of n points in n_rooms rooms (an upper bound of the summed capacities)
static inline long lrg_room_hash_slots(long n, long n_rooms) { return 4L * n + 64L * n_rooms; }

// Bounds of room r (room_start was checked on the host: this only keeps a bad word from turning into an address)
__device__ __forceinline__ bool lrg_room_bounds(const int32_t *room_start, int n, int r, int *s, int *e) {
    const int s0 = room_start[r], e0 = room_start[r + 1];
    if (s0 < 0 || e0 < s0 || e0 > n) return false;
    *s = s0; *e = e0;
    return true;
}

// the segment of room r = points s .. e - 1: its first slot and its mask
__device__ __forceinline__ void lrg_room_segment(int r, int s, int e, long *off, int *mask) {
    int cap = 64;
    while (cap < 2 * (e - s)) cap <<= 1;
    *off = 4L * s + 64L * r;
    *mask = cap - 1;
}

// ... as pointers into a key array and one array of values
__device__ __forceinline__ void lrg_room_segment(uint64_t *keys, int32_t *vals, int r, int s, int e, uint64_t **seg_keys, int32_t **seg_vals,
                                                 int *mask) {
    long off;
    lrg_room_segment(r, s, e, &off, mask);
    *seg_keys = keys + off; *seg_vals = vals + off;
}

// the room of point i (empty rooms are skipped)
__device__ __forceinline__ int lrg_room_of(const int32_t *room_start, int n_rooms, int i) { return lrg_last_start(room_start, 0, n_rooms - 1, i); }

// The slot of `key` in a segment, claimed by CAS if the key is not there yet; *claimed (nullable) = this call put the key in.  -1 after
// mask + 1 probes without an empty slot or the key (never: a segment has >= 2 n_room slots).
__device__ __forceinline__ int lrg_room_claim(uint64_t *keys, int mask, uint64_t key, bool *claimed = nullptr) {
    unsigned h = (unsigned)lrg_fmix64(key) & (unsigned)mask;
    for (int probe = 0; probe <= mask; ++probe) {
        const unsigned long long prev = atomicCAS(reinterpret_cast<unsigned long long *>(&keys[h]), (unsigned long long)LRG_HASH_EMPTY,
                                                  (unsigned long long)key);
        if (prev == LRG_HASH_EMPTY || prev == key) {
            if (claimed) *claimed = prev == LRG_HASH_EMPTY;
            return (int)h;
        }
        h = (h + 1) & (unsigned)mask;
    }
    return -1;
}

// The slot of `key` in a segment, -1 when absent.  (With one array of values lrg_hash_lookup loads key and value together.)
__device__ __forceinline__ int lrg_room_find(const uint64_t *keys, int mask, uint64_t key) {
    if (key == LRG_HASH_EMPTY) return -1;
    unsigned h = (unsigned)lrg_fmix64(key) & (unsigned)mask;
    for (int probe = 0; probe <= mask; ++probe) {
        const uint64_t k = keys[h];
        if (k == key) return (int)h;
        if (k == LRG_HASH_EMPTY) return -1;
        h = (h + 1) & (unsigned)mask;
    }
    return -1;
}

// key -> i in the room's segment; false when the key is there already (two points of the room in one voxel)
__device__ __forceinline__ bool lrg_room_insert(uint64_t *keys, int32_t *vals, int mask, uint64_t key, int i) {
    bool claimed = false;
    const int h = lrg_room_claim(keys, mask, key, &claimed);
    if (claimed) vals[h] = i;
    return h < 0 || claimed;
}
