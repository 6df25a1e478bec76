// ABI 22.  Training tuples for LrgNet on the device: the imperfect teacher of stage_data.py:104-231 under the counter stream
// (lrg_stage_teacher: one workgroup per room, a chain of small steps, integer decisions only) and the rows of its tuples centred on the
// medians of the emitted inlier side (lrg_stage_tuples: one workgroup per tuple, stage_data.py:233-240).  No workgroup waits for another
// and every loop is bounded: the seed search by the room's points, an object's passes by max_iters, a room's output by its arena.
#include "lrg_common.h"
#include "lrg_rng.h"
#include "lrg_median.h"

#define LRG_STAGE_BT 1024
#define LRG_STAGE_PER_THREAD 4                       // consecutive points of one thread per chunk: one ordered compaction per 4096 points
#define LRG_STAGE_FLAG 0x80000000u                   // list entry: the point's remove / add flag (rejectClass / expandClass, :152,:163)
#define LRG_STAGE_DECIDE 0x40000000u                 // list entry (lists only, never emitted): the teacher's decision, flag xor mistake (:159,:170)
#define LRG_STAGE_INDEX 0x3FFFFFFFu

namespace {

struct StageShared {
    int wave_a[LRG_STAGE_BT / 64], wave_b[LRG_STAGE_BT / 64];
    int red[8];
};

// Sums of three per-thread counters over the workgroup, returned to every thread.
__device__ __forceinline__ void stage_block_sum3(int &a, int &b, int &c, int *red) {
    a = lrg_wave_sum_i32(a); b = lrg_wave_sum_i32(b); c = lrg_wave_sum_i32(c);
    if (threadIdx.x < 3) red[threadIdx.x] = 0;
    __syncthreads();
    if (lrg_lane() == 0) { if (a) atomicAdd(&red[0], a); if (b) atomicAdd(&red[1], b); if (c) atomicAdd(&red[2], c); }
    __syncthreads();
    a = red[0]; b = red[1]; c = red[2];
    __syncthreads();
}

__device__ __forceinline__ int stage_wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int stage_wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// (word >> 8) * 100 < p100 << 24: a mistake with probability p100 / 100 on the 24-bit uniform, in integers
__device__ __forceinline__ bool stage_mistake(uint32_t w, int p100) {
    return (uint64_t)(w >> 8) * 100ull < ((uint64_t)p100 << 24);
}

__global__ __launch_bounds__(LRG_STAGE_BT) void lrg_stage_teacher_kernel(
    const LrgRoom *rooms, const int32_t *room_list, const int64_t *ws_off, uint8_t *cur_mask, int32_t *lists, int32_t *arena_base,
    const int64_t *arena_off, const int32_t *arena_cap, int32_t *objects, int32_t *status, uint32_t rng_seed, int max_points,
    int cluster_threshold, int max_steps, int max_iters) {
    __shared__ StageShared sh;
    const int tid = threadIdx.x, lane = lrg_lane(), wave = tid >> 6;
    constexpr int NW = LRG_STAGE_BT / 64, CHUNK = LRG_STAGE_BT * LRG_STAGE_PER_THREAD;
    const int r = room_list[blockIdx.x];
    const LrgRoom R = rooms[r];
    const int n = R.n;
    const int32_t *vox = R.voxels, *obj = R.obj_id;
    uint8_t *visited = R.visited, *cur = cur_mask + ws_off[r];
    uint32_t *cur_list = reinterpret_cast<uint32_t *>(lists) + 2 * ws_off[r], *cand_list = cur_list + n;
    uint32_t *arena = reinterpret_cast<uint32_t *>(arena_base) + arena_off[r];
    int32_t *obj_out = objects + 4 * ws_off[r];
    const int cap = arena_cap[r];
    const uint32_t k0 = rng_seed, k1 = (uint32_t)R.room_id;

    for (int i = tid; i < n; i += LRG_STAGE_BT) { visited[i] = 0; cur[i] = 0; }
    __syncthreads();

    // seed order (:107): the Feistel permutation of the room's points
    lrg_u32x4 seed_keys = lrg_philox4x32_10(0u, 0u, 0u, LRG_PURPOSE_PERMKEY | LRG_PURPOSE_STAGE_SEED, k0, k1);
    int room_status = LRG_STAGE_OK, n_tuples = 0, used = 0, n_objects = 0;
    int k = 0;                                                   // position in the seed order
    while (k < n && room_status == LRG_STAGE_OK) {
        // ---- the next unvisited seed: LRG_STAGE_BT positions of the order at once (:109-110) ----
        {
            const int kk = k + tid;
            int found = INT_MAX;
            if (kk < n) {
                const int sd = n == 1 ? 0 : (int)lrg_feistel_permute((uint32_t)kk, (uint32_t)n, seed_keys);
                if (!visited[sd]) found = kk;
            }
            found = stage_wave_min(found);
            if (tid == 0) sh.red[0] = INT_MAX;
            __syncthreads();
            if (lane == 0 && found != INT_MAX) atomicMin(&sh.red[0], found);
            __syncthreads();
            found = sh.red[0];
            __syncthreads();
            if (found == INT_MAX) { k += LRG_STAGE_BT; continue; }
            k = found + 1;
        }
        const int s = n == 1 ? 0 : (int)lrg_feistel_permute((uint32_t)(k - 1), (uint32_t)n, seed_keys);
        const int target = obj[s];
        int gt = 0;
        {
            int z0 = 0, z1 = 0;
            for (int i = tid; i < n; i += LRG_STAGE_BT) gt += obj[i] == target ? 1 : 0;
            stage_block_sum3(gt, z0, z1, sh.red);
        }
        if (tid == 0) cur[s] = 1;                                // :122-125
        int mn0 = vox[3 * s], mn1 = vox[3 * s + 1], mn2 = vox[3 * s + 2], mx0 = mn0, mx1 = mn1, mx2 = mn2;
        int steps = 0, stuck = 0;
        int p_add = 10 * (2 + (int)(((uint64_t)lrg_rng_word(0u, LRG_PURPOSE_STAGE_PROB, (uint32_t)s, 0u, 0u, k0, k1) * 3ull) >> 32));   // :128
        int p_rmv = 10 * (2 + (int)(((uint64_t)lrg_rng_word(1u, LRG_PURPOSE_STAGE_PROB, (uint32_t)s, 0u, 0u, k0, k1) * 3ull) >> 32));   // :129
        __syncthreads();
        for (int t = 0;; ++t) {                                  // :138
            if (t >= max_iters) { room_status = LRG_STAGE_ITER_CAP; break; }
            // ---- both lists in point-index order (:141-171): flags, the teacher's decisions, the counts ----
            int nc = 0, ne = 0, inter = 0, nexp = 0, nrej = 0;
            for (int base = 0; base < n; base += CHUNK) {
                const int i0 = base + tid * LRG_STAGE_PER_THREAD;
                uint32_t ent[LRG_STAGE_PER_THREAD];
                int kind[LRG_STAGE_PER_THREAD];                  // 0 neither, 1 current, 2 candidate
                int a = 0, b = 0;
#pragma unroll
                for (int q = 0; q < LRG_STAGE_PER_THREAD; ++q) {
                    const int i = i0 + q;
                    kind[q] = 0; ent[q] = 0u;
                    if (i >= n) continue;
                    if (cur[i]) {
                        const bool rej = obj[i] != target;                                                       // :163
                        bool dec = rej;
                        if (!stuck) dec ^= stage_mistake(lrg_rng_word((uint32_t)i, LRG_PURPOSE_STAGE_RMV, (uint32_t)s, 0u, (uint32_t)t, k0, k1), p_rmv);
                        kind[q] = 1; ++a;
                        inter += rej ? 0 : 1; nrej += dec ? 1 : 0;
                        ent[q] = (uint32_t)i | (rej ? LRG_STAGE_FLAG : 0u) | (dec ? LRG_STAGE_DECIDE : 0u);
                    } else if (!visited[i]) {
                        const int v0 = vox[3 * i], v1 = vox[3 * i + 1], v2 = vox[3 * i + 2];
                        if (v0 >= mn0 - 1 && v0 <= mx0 + 1 && v1 >= mn1 - 1 && v1 <= mx1 + 1 && v2 >= mn2 - 1 && v2 <= mx2 + 1) {     // :146
                            const bool ex = obj[i] == target;                                                    // :152
                            bool dec = ex;
                            if (!stuck) dec ^= stage_mistake(lrg_rng_word((uint32_t)i, LRG_PURPOSE_STAGE_ADD, (uint32_t)s, 0u, (uint32_t)t, k0, k1), p_add);
                            kind[q] = 2; ++b;
                            nexp += ex ? 1 : 0;
                            ent[q] = (uint32_t)i | (ex ? LRG_STAGE_FLAG : 0u) | (dec ? LRG_STAGE_DECIDE : 0u);
                        }
                    }
                }
                const int ia = lrg_wave_incl_scan_i32(a), ib = lrg_wave_incl_scan_i32(b);
                if (lane == 63) { sh.wave_a[wave] = ia; sh.wave_b[wave] = ib; }
                __syncthreads();
                int pa = nc + ia - a, pb = ne + ib - b;
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    const int wa = sh.wave_a[w], wb = sh.wave_b[w];
                    if (w < wave) { pa += wa; pb += wb; }
                    nc += wa; ne += wb;
                }
#pragma unroll
                for (int q = 0; q < LRG_STAGE_PER_THREAD; ++q) {
                    if (kind[q] == 1) cur_list[pa++] = ent[q];             // pa < nc <= n, pb < ne <= n
                    else if (kind[q] == 2) cand_list[pb++] = ent[q];
                }
                __syncthreads();
            }
            stage_block_sum3(inter, nexp, nrej, sh.red);                   // (the barriers inside publish the lists to the workgroup)
            bool any_rej = inter < nc, any_exp = nexp > 0;
            // ---- one tuple (:173-199) ----
            if (ne > 0) {
                const int ae = min(nc, max_points), be = min(ne, max_points);
                if ((long)used + ae + be + 8l * (n_tuples + 1) > (long)cap) { room_status = LRG_STAGE_OVERFLOW; break; }
                int cnt_r = 0, cnt_e = 0, z = 0;
                const lrg_u32x4 kin = lrg_philox4x32_10(0u, (uint32_t)t, (uint32_t)s, LRG_PURPOSE_PERMKEY | LRG_PURPOSE_STAGE_INLIER, k0, k1);
                const lrg_u32x4 knb = lrg_philox4x32_10(0u, (uint32_t)t, (uint32_t)s, LRG_PURPOSE_PERMKEY | LRG_PURPOSE_STAGE_NEIGHBOR, k0, k1);
                for (int j = tid; j < ae; j += LRG_STAGE_BT) {
                    const uint32_t e = cur_list[nc > max_points ? lrg_feistel_permute((uint32_t)j, (uint32_t)nc, kin) : (uint32_t)j];
                    arena[used + j] = e & ~LRG_STAGE_DECIDE;
                    cnt_r += (int)(e >> 31);
                }
                for (int j = tid; j < be; j += LRG_STAGE_BT) {
                    const uint32_t e = cand_list[ne > max_points ? lrg_feistel_permute((uint32_t)j, (uint32_t)ne, knb) : (uint32_t)j];
                    arena[used + ae + j] = e & ~LRG_STAGE_DECIDE;
                    cnt_e += (int)(e >> 31);
                }
                stage_block_sum3(cnt_r, cnt_e, z, sh.red);
                any_rej = cnt_r > 0;                             // :182, :192: the flags are reassigned to the subsample
                any_exp = cnt_e > 0;
                if (tid == 0) {
                    uint32_t *h = arena + cap - 8 * (n_tuples + 1);
                    h[0] = (uint32_t)ae; h[1] = (uint32_t)be; h[2] = (uint32_t)used; h[3] = (uint32_t)(used + ae);
                    h[4] = __float_as_uint((float)((double)inter / (double)(nc + gt - inter)));      // :194, two roundings as NumPy's
                    h[5] = (uint32_t)s; h[6] = (uint32_t)t; h[7] = 0u;
                }
                used += ae + be; ++n_tuples; ++steps;
                p_add = max(p_add - 1, 0); p_rmv = max(p_rmv - 1, 0);                               // :198-199
            }
            const bool complete = inter == nc && nc == gt;       // :201
            const bool go_on = !complete && steps < max_steps && (any_exp || any_rej);              // :209
            if (!go_on) {
                const bool store = complete || nc > cluster_threshold;                              // :225
                for (int j = tid; j < nc; j += LRG_STAGE_BT) {
                    const int i = (int)(cur_list[j] & LRG_STAGE_INDEX);
                    cur[i] = 0;
                    if (store) visited[i] = 1;
                }
                if (store) {
                    if (tid == 0) {
                        int32_t *o = obj_out + 4 * n_objects;
                        o[0] = steps; o[1] = s; o[2] = nc;
                        o[3] = (int32_t)__float_as_uint((float)((double)inter / (double)(nc + gt - inter)));
                    }
                    ++n_objects;
                }
                __syncthreads();
                break;
            }
            // ---- the teacher's update (:212-223) and the new bounding box ----
            const bool remove = nrej < nc;                       // :213
            int b0 = INT_MAX, b1 = INT_MAX, b2 = INT_MAX, t0 = INT_MIN, t1 = INT_MIN, t2 = INT_MIN;
            for (int j = tid; j < nc; j += LRG_STAGE_BT) {
                const uint32_t e = cur_list[j];
                const int i = (int)(e & LRG_STAGE_INDEX);
                if (remove && (e & LRG_STAGE_DECIDE)) { cur[i] = 0; continue; }
                const int v0 = vox[3 * i], v1 = vox[3 * i + 1], v2 = vox[3 * i + 2];
                b0 = min(b0, v0); b1 = min(b1, v1); b2 = min(b2, v2); t0 = max(t0, v0); t1 = max(t1, v1); t2 = max(t2, v2);
            }
            for (int j = tid; j < ne; j += LRG_STAGE_BT) {
                const uint32_t e = cand_list[j];
                if (!(e & LRG_STAGE_DECIDE)) continue;
                const int i = (int)(e & LRG_STAGE_INDEX);
                cur[i] = 1;
                const int v0 = vox[3 * i], v1 = vox[3 * i + 1], v2 = vox[3 * i + 2];
                b0 = min(b0, v0); b1 = min(b1, v1); b2 = min(b2, v2); t0 = max(t0, v0); t1 = max(t1, v1); t2 = max(t2, v2);
            }
            b0 = stage_wave_min(b0); b1 = stage_wave_min(b1); b2 = stage_wave_min(b2);
            t0 = stage_wave_max(t0); t1 = stage_wave_max(t1); t2 = stage_wave_max(t2);
            if (tid < 6) sh.red[tid] = tid < 3 ? INT_MAX : INT_MIN;
            __syncthreads();
            if (lane == 0) {
                atomicMin(&sh.red[0], b0); atomicMin(&sh.red[1], b1); atomicMin(&sh.red[2], b2);
                atomicMax(&sh.red[3], t0); atomicMax(&sh.red[4], t1); atomicMax(&sh.red[5], t2);
            }
            __syncthreads();
            b0 = sh.red[0]; b1 = sh.red[1]; b2 = sh.red[2]; t0 = sh.red[3]; t1 = sh.red[4]; t2 = sh.red[5];
            __syncthreads();
            if (!(b0 < mn0 || b1 < mn1 || b2 < mn2) && !(t0 > mx0 || t1 > mx1 || t2 > mx2)) stuck = 1;      // :217, never cleared
            mn0 = b0; mn1 = b1; mn2 = b2; mx0 = t0; mx1 = t1; mx2 = t2;
        }
    }
    if (tid == 0) {
        status[4 * r] = room_status; status[4 * r + 1] = n_tuples; status[4 * r + 2] = used; status[4 * r + 3] = n_objects;
    }
}

// One tuple: medians of the centred channels over the emitted inlier rows (one wavefront per channel, 16 keys per lane in registers),
// then both sides gathered and centred in float32 (stage_data.py:233-240).
__global__ __launch_bounds__(LRG_STAGE_BT) void lrg_stage_tuples_kernel(const LrgRoom *rooms, const int32_t *arena_base, const int32_t *table, int F,
                                                                        float *points, int32_t *remove, float *neighbor_points, int32_t *add) {
    __shared__ float med[LRG_STAGE_MAX_FEATURES];
    const int tid = threadIdx.x, lane = lrg_lane(), wave = tid >> 6;
    const int32_t *row = table + 8 * (long)blockIdx.x;
    const int a = row[1], b = row[2];
    const float *pts = rooms[row[0]].points;
    const uint32_t *ein = reinterpret_cast<const uint32_t *>(arena_base) + row[3], *enb = reinterpret_cast<const uint32_t *>(arena_base) + row[4];
    const long out_in = row[5], out_nb = row[6];
    const int n_centred = 2 + max(F - 6, 0);
    for (int y = wave; y < n_centred; y += LRG_STAGE_BT / 64) {
        const int ch = y < 2 ? y : y + 4;
        uint32_t key[16];
        int id[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) id[q] = (int)(ein[min(q * 64 + lane, a - 1)] & LRG_STAGE_INDEX);
#pragma unroll
        for (int q = 0; q < 16; ++q) key[q] = (q * 64 + lane < a) ? lrg_f2key(pts[(long)id[q] * F + ch]) : 0xFFFFFFFFu;
        const float m = lrg_select_regs<16>(key, a);
        if (lane == 0) med[ch] = m;
    }
    __syncthreads();
    for (int x = tid; x < a * F; x += LRG_STAGE_BT) {
        const int j = x / F, c = x - j * F;
        const uint32_t e = ein[j];
        float v = pts[(long)(e & LRG_STAGE_INDEX) * F + c];
        if (c < 2 || c >= 6) v = __fsub_rn(v, med[c]);
        points[(out_in + j) * F + c] = v;
        if (c == 0) remove[out_in + j] = (int32_t)(e >> 31);
    }
    for (int x = tid; x < b * F; x += LRG_STAGE_BT) {
        const int j = x / F, c = x - j * F;
        const uint32_t e = enb[j];
        float v = pts[(long)(e & LRG_STAGE_INDEX) * F + c];
        if (c < 2 || c >= 6) v = __fsub_rn(v, med[c]);
        neighbor_points[(out_nb + j) * F + c] = v;
        if (c == 0) add[out_nb + j] = (int32_t)(e >> 31);
    }
}

}  // namespace

extern "C" {

int lrg_stage_teacher(const LrgRoom *rooms, const int32_t *room_list, int n_list, const int64_t *ws_off, uint8_t *cur_mask, int32_t *lists,
                      int32_t *arena, const int64_t *arena_off, const int32_t *arena_cap, int32_t *objects, int32_t *status, uint32_t rng_seed,
                      int max_points, int cluster_threshold, int max_steps, int max_iters, void *stream) {
    if (!rooms || !room_list || !ws_off || !cur_mask || !lists || !arena || !arena_off || !arena_cap || !objects || !status) return LRG_EINVAL - 100;
    if (n_list < 1 || n_list > (1 << 20)) return LRG_EINVAL - 101;
    if (max_points < 1 || max_points > LRG_STAGE_MAX_POINTS) return LRG_EINVAL - 102;
    if (max_steps < 0 || max_iters < 1 || cluster_threshold < 0) return LRG_EINVAL - 103;
    hipLaunchKernelGGL(lrg_stage_teacher_kernel, dim3(n_list), dim3(LRG_STAGE_BT), 0, (hipStream_t)stream, rooms, room_list, ws_off, cur_mask, lists,
                       arena, arena_off, arena_cap, objects, status, rng_seed, max_points, cluster_threshold, max_steps, max_iters);
    LRG_LAUNCH_CHECK();
    return 0;
}

int lrg_stage_tuples(const LrgRoom *rooms, const int32_t *arena, const int32_t *table, int n_tuples, int F, float *points, int32_t *remove,
                     float *neighbor_points, int32_t *add, void *stream) {
    if (!rooms || !arena || !table || !points || !remove || !neighbor_points || !add) return LRG_EINVAL - 105;
    if (n_tuples < 1) return LRG_EINVAL - 106;
    if (F < 3 || F > LRG_STAGE_MAX_FEATURES) return LRG_EINVAL - 107;
    hipLaunchKernelGGL(lrg_stage_tuples_kernel, dim3(n_tuples), dim3(LRG_STAGE_BT), 0, (hipStream_t)stream, rooms, arena, table, F, points, remove,
                       neighbor_points, add);
    LRG_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
