// The pooled-product units of the free-running launch (lrg_grow_async): workgroups of the front kernel that keep the heads' first-layer kernels on chip and
// turn a slot's pooled row into its 2 x 256 sums.  Three forms of one role -- four teams of four wavefronts, eight half-teams, and the slice in registers --
// with one interface: the ring every unit reads, the slot's pooled row (or per-tile pool rows), 32 sums per (slot, unit) and one arrival on sync[1].
// Included by lrg_async.inl, and by tools/wave_tile_probe.hip, which runs each form alone (mode `units`).  The includer has lrg_async_plan.h and defines
// LRG_FRONT_THREADS, LRG_ASYNC_SYNC_WORDS, LRG_TASK_GEMV, LRG_DBG / lrg_dbg_add and lrg_drain_stores before this file.

// ---- the launch's arguments ----
// ONE kernel parameter, LrgAsyncKArgs (lrg_async_plan.h, where the reasons are)
// (inside a non-kernel function __builtin_amdgcn_kernarg_segment_ptr() folds to null: the kernel takes the pointer and hands it on,
//  typed as constant address space, so that the roles' loads of the arguments stay scalar loads)
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) void *lrg_kargs_ptr;
#else
typedef const void *lrg_kargs_ptr;
#endif
#define LRG_ASYNC_KARGS() (*(const LrgAsyncKArgs *)kp)
// Arguments of a non-kernel function arrive in vector registers; what is wave-uniform goes back to scalar registers first, so that
// the loads of the launch's arguments are scalar loads and the addresses derived from them scalar arithmetic.
__device__ __forceinline__ lrg_kargs_ptr lrg_uniform(lrg_kargs_ptr p) {
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (lrg_kargs_ptr)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ int lrg_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
// the launch's dynamic LDS: roles get OFFSETS into it (a float * parameter would be a generic pointer, and every LDS access of a
// tile a flat instruction)
extern __shared__ __attribute__((aligned(16))) float lrg_async_smem[];
#include "lrg_wave_tile.inl"
#define LRG_ASYNC_ROLE __device__ __noinline__

// ---- pooled-product units: the heads' pooled kernels stay in LDS ----
// As a task of the tile teams the pooled product of a slot is four trips of 512 KB from L2 (7.7 us each, 12.5 us from the last branch
// tile to the last block with the queueing, profiles/r03_free8_perf.log) in the middle of the slot's chain of latencies.  The
// kernels are the same for every slot: 2 x [P = 1024, C = 256] floats = 2 MB = sixteen CUs' LDS at 32 columns each.  A unit
// (workgroup) loads its [P, 32] slice once per launch; its four teams of four wavefronts take the slots whose branch tiles have
// all arrived from ONE ring that every unit reads (entry i: (generation of i) << 20 | slot, written once by the last branch tile
// to arrive; a unit's teams take the entries in turn -- a ticket counter in the unit's LDS, nothing to reserve in memory); a task =
// the slot's 4 KB pooled row from L2, 128 FMAs per lane from LDS, 32 sums out, one more arrival on the slot's pooled-product counter,
// which the slot's head tiles poll (LrgWaitPooled).  Summation order: that of lrg_head_gemv_kernel (eight K ranges, MFMA k order
// inside, the partial sums in order, the bias last) -- bit for bit what the tile teams' blocks give.
// (Tried: mailboxes instead of the ring -- a 64-bit word per slot, arrivals | target << 32, every branch tile adds itself, one team per
// unit watches all slots -- so that the units start ~2 us earlier, before the last tile knows it was the last: 808 k -> 795 k
// instance-steps/s at 68 slots, the second atomic per tile and the watchers' loads cost more than the earlier start gains.)
#define LRG_GEMV_UNIT_COLS 32
#define LRG_GEMV_UNIT_TEAMS 4
#define LRG_GEMV_UNIT_TEAM_FLOATS(P) ((P) + 8 * LRG_GEMV_UNIT_COLS + 16)      // pooled row, partial sums, task words + barrier counter
#define LRG_GEMV_UNIT_FLOATS(P) ((P) * LRG_GEMV_UNIT_COLS + LRG_GEMV_UNIT_TEAMS * LRG_GEMV_UNIT_TEAM_FLOATS(P))      // + n_slots claim words behind
#define LRG_GEMV_UNIT_MAX_SLOTS 2048
__device__ __forceinline__ int lrg_gemv_ring_tag(int i, int gmask) { return (((unsigned)i / (unsigned)(gmask + 1)) % 2047u) + 1; }

// ---- a pooled-product unit (see LRG_GEMV_UNIT_COLS above): `unit` = 0 .. gemv_units - 1, all sixteen wavefronts arrive here ----
LRG_ASYNC_ROLE void lrg_async_gemv_unit(lrg_kargs_ptr kp_, int unit_, long long t_launch) {
    const lrg_kargs_ptr kp = lrg_uniform(kp_);
    const int unit = lrg_uniform(unit_);
    const LrgAsyncArgs &A = LRG_ASYNC_KARGS().A;
    const LrgGemvArgs &g = A.gemv;
    const int P = g.P, kq = P >> 3;
    const int upz = g.C / LRG_GEMV_UNIT_COLS;                 // units per head
    const int z = unit / upz, col0 = (unit - z * upz) * LRG_GEMV_UNIT_COLS;
    float *wl = lrg_async_smem;                                // [P][32] this unit's columns of head z's pooled kernel
    {   // the slice, once per launch: 16-byte loads, eight per row
        const float *w = g.w[z] + col0;
        for (int i = threadIdx.x; i < P * (LRG_GEMV_UNIT_COLS / 4); i += LRG_FRONT_THREADS) {
            const int row = i >> 3, q = i & 7;
            *reinterpret_cast<float4 *>(wl + row * LRG_GEMV_UNIT_COLS + 4 * q) = *reinterpret_cast<const float4 *>(w + (long)row * g.ldw + 4 * q);
        }
    }
    const int t = lrg_uniform((int)threadIdx.x >> 8);
    float *sm = lrg_async_smem + P * LRG_GEMV_UNIT_COLS + t * LRG_GEMV_UNIT_TEAM_FLOATS(P);
    float *pl = sm, *part = sm + P;
    int *word = reinterpret_cast<int *>(part + 8 * LRG_GEMV_UNIT_COLS);      // [0], [1] the task of even / odd rounds, [4] barrier counter
    int *ctl = reinterpret_cast<int *>(lrg_async_smem + LRG_GEMV_UNIT_FLOATS(P));          // [0] the unit's next ring entry
    if ((threadIdx.x & 255) == 0) { word[0] = 0; word[1] = 0; word[4] = 0; }
    if (threadIdx.x < 4) ctl[threadIdx.x] = 0;
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                              // the slice is in place; from here on the teams go their own ways
    LrgLdsTeam team;
    team.cnt = &word[4];
    team.target = 0;
    team.base = (int)(threadIdx.x & ~255u);
    team.gave_up = &A.queue[LRG_AQ_ABORT];
    const int tid = team.tid(), lane = tid & 63, wave = tid >> 6;
    const int c = lane & 31, r = 2 * wave + (lane >> 5);      // this lane's column and K range
    const float bias = g.bias[z] ? g.bias[z][col0 + (tid & 31)] : 0.f;
    const int32_t *ring = A.queue + LRG_AQ_RING + 2 * (A.qmask + 1);
    for (int round = 0;; round ^= 1) {
        long long t_task = 0;
        if (wave == 0) {
            // the unit's next ring entry, taken by whichever team is free; the other wavefronts wait at the barrier below
            int slot = -2;
            int i = 0;
            if (lane == 0) i = __hip_atomic_fetch_add(&ctl[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            i = __shfl(i, 0);
            const int32_t *e = ring + (i & A.gmask);
            const int tag = lrg_gemv_ring_tag(i, A.gmask);
            for (unsigned spin = 0; slot == -2; ++spin) {
                const int code = lrg_ld_coh(e);
                if ((code >> 20) == tag) { slot = code & 0xFFFFF; break; }      // (slot | tile counts: unpacked below)
                if ((spin & 7) == 7) {
                    if (lrg_ld_coh(&A.queue[LRG_AQ_FRONTS_DONE]) >= A.n_front || lrg_ld_coh(&A.queue[LRG_AQ_ABORT])) slot = -1;
                    else if ((spin & 1023) == 1023 && wall_clock64() - t_launch > A.abort_ticks) {
                        lrg_st_coh(&A.queue[LRG_AQ_ABORT], 4);
                        slot = -1;
                    }
                }
                if (slot == -2) __builtin_amdgcn_s_sleep(2);
            }
            if (lane == 0) word[round] = slot;
        }
        team.sync();
        const int entry = word[round];                        // (the other word is written next round: no second barrier)
        if (entry < 0) return;
        const int slot = entry & 0xFFF;                       // (units serve at most LRG_GEMV_UNIT_MAX_SLOTS = 2048 slots)
        if (LRG_DBG(A)) t_task = wall_clock64();
        if (A.pool_rows) {
            // the slot's pooled feature (:122-125) = the maximum over its branch tiles' rows of column maxima, taken here on the way into LDS:
            // every lane owns 16 bytes of the feature and has one load per tile of that side in flight (the values are >= 0: their
            // order is that of their bit patterns, as in the atomicMax formulation)
            const int nt_in = ((entry >> 16) & 15) + 1, nt_nb = ((entry >> 12) & 15) + 1;
            const int half4 = P >> 3;                          // 16-byte pieces per side
            const float *rows = A.pool_rows + (long)slot * A.pool_rows_stride;
            for (int j = tid; j < (P >> 2); j += FTHREADS) {
                const int side = j >= half4 ? 1 : 0, c4 = j - side * half4, nt = side ? nt_nb : nt_in;
                const float *src = rows + (long)side * 16 * (P >> 1);
                int4 m = make_int4(0, 0, 0, 0);
                for (int t0 = 0; t0 < nt; t0 += 8) {          // (eight loads in flight: a side has 3.5 tiles on average, 16 at most)
                    float4 v[8];
#pragma unroll
                    for (int t = 0; t < 8; ++t)
                        if (t0 + t < nt) v[t] = lrg_ld_coh4(src, (unsigned)((t0 + t) * (P >> 1) + 4 * c4) * 4u);
#pragma unroll
                    for (int t = 0; t < 8; ++t)
                        if (t0 + t < nt) {
                            m.x = max(m.x, __float_as_int(v[t].x)); m.y = max(m.y, __float_as_int(v[t].y));
                            m.z = max(m.z, __float_as_int(v[t].z)); m.w = max(m.w, __float_as_int(v[t].w));
                        }
                }
                *reinterpret_cast<int4 *>(pl + 4 * j) = m;
            }
        } else {   // the slot's pooled row: one 16-byte load per lane
#ifndef LRG_EXP_NO_UNIT_LOAD      // (experiment switch, --policy gt only)
            const float *src = g.pooled + (long)slot * P;
            for (int j = tid; j < (P >> 2); j += FTHREADS)
                *reinterpret_cast<float4 *>(pl + 4 * j) = lrg_ld_coh4(src, (unsigned)j * 16u);
#endif
        }
        team.sync();
        {
            const float *w = wl + (r * kq) * LRG_GEMV_UNIT_COLS + c;
            const float *p = pl + r * kq;
            float acc = 0.f;
            for (int kb = 0; kb < kq; kb += 16) {
                float wv[16];
                float4 pv[4];
#pragma unroll
                for (int u = 0; u < 16; ++u) wv[u] = w[(kb + u) * LRG_GEMV_UNIT_COLS];
#pragma unroll
                for (int u = 0; u < 4; ++u) pv[u] = *reinterpret_cast<const float4 *>(p + kb + 4 * u);
                const float pk[16] = {pv[0].x, pv[0].y, pv[0].z, pv[0].w, pv[1].x, pv[1].y, pv[1].z, pv[1].w,
                                      pv[2].x, pv[2].y, pv[2].z, pv[2].w, pv[3].x, pv[3].y, pv[3].z, pv[3].w};
#pragma unroll
                for (int uu = 0; uu < 16; ++uu) {
                    const int u = (uu & 8) | ((uu & 1) << 2) | ((uu >> 1) & 3);      // k = 8g + 0, 4, 1, 5, 2, 6, 3, 7 (lrg_async_gemv)
                    acc = fmaf(pk[u], wv[u], acc);
                }
            }
            part[r * LRG_GEMV_UNIT_COLS + c] = acc;
        }
        team.sync();
        // the sums and the arrival by the LAST wavefront: the first is back at the mailboxes while these stores drain
        if (wave == 3) {
            {   // (32 sums, stored as eight 16-byte pieces)
                float sum = part[lane & (LRG_GEMV_UNIT_COLS - 1)];
#pragma unroll
                for (int q = 1; q < 8; ++q) sum += part[q * LRG_GEMV_UNIT_COLS + (lane & (LRG_GEMV_UNIT_COLS - 1))];
                sum += bias;
                const float v0 = __shfl(sum, 4 * (lane & 7)), v1 = __shfl(sum, 4 * (lane & 7) + 1), v2 = __shfl(sum, 4 * (lane & 7) + 2), v3 = __shfl(sum, 4 * (lane & 7) + 3);
                if (lane < LRG_GEMV_UNIT_COLS / 4) lrg_st_coh4(g.hb[z] + (long)slot * g.C + col0, (unsigned)lane * 16u, make_float4(v0, v1, v2, v3));
            }
            lrg_drain_stores();
            if (lane == 0) {
                int32_t *sy = A.sync + (long)slot * LRG_ASYNC_SYNC_WORDS;
                if (LRG_DBG(A)) {
                    const int done = __hip_atomic_fetch_add(&sy[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
                    const long long now = wall_clock64();
                    lrg_dbg_add(A, 8 + 2 * LRG_TASK_GEMV, now - t_task); lrg_dbg_add(A, 9 + 2 * LRG_TASK_GEMV, 1);
                    if (done == lrg_ld_coh(&sy[5])) lrg_dbg_add(A, 3, (int)((unsigned)now - (unsigned)lrg_ld_coh(&sy[8])));
                } else {
                    __hip_atomic_fetch_add(&sy[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    }
}

// ---- a pooled-product unit of HALF-TEAMS (round 6): eight tasks in flight per unit instead of four ----
// With the register tiles a step is ~69 us and sixteen units x four teams x 3.3 us a task are 81 % busy at 0.99 M evaluations a second: a slot's pooled product
// queues for the slowest of its sixteen units (15 us from the last branch tile to the last sum, profiles/r06_bench_debug_68_reg_tiles.log).  A task's 3.3 us are
// latencies (the ring entry, the slot's pooled row, two barriers, the store, the arrival), not arithmetic, and a fifth team has no place: four staged rows are all the
// LDS holds beside the unit's 128 KB slice.  Here a task is run by TWO wavefronts: the row comes in ONE trip (16 bytes of either half per thread) and is staged half
// at a time (2 KB); a lane owns a column and TWO of the eight K ranges (256 FMAs).  Eight half-teams = sixteen wavefronts: twice the tasks in flight on the same LDS.
// (First form: no staging, the row's values read chunk by chunk with write-through-coherent loads one chunk ahead -- sixteen dependent trips to the memory side per
//  task: 15 us a task, 530 k instance-steps/s.)  The sums are those of lrg_async_gemv_unit bit for bit (per K range a chain
// over k = 8g + 0, 4, 1, 5, 2, 6, 3, 7; the eight partial sums in order; the bias last).
#define LRG_GEMV_UNIT2_TEAM_FLOATS(P) ((P) / 2 + 8 * LRG_GEMV_UNIT_COLS + 32)      // half a pooled row, partial sums, task words + barrier counter
#define LRG_GEMV_UNIT2_FLOATS(P) ((P) * LRG_GEMV_UNIT_COLS + 8 * LRG_GEMV_UNIT2_TEAM_FLOATS(P) + 4)
// (LrgLdsPair, the two wavefronts' meeting: lrg_fused_tile.inl, beside LrgLdsTeam -- the register branch tiles' wave pairs use it too)

LRG_ASYNC_ROLE void lrg_async_gemv_unit2(lrg_kargs_ptr kp_, int unit_, long long t_launch) {
    const lrg_kargs_ptr kp = lrg_uniform(kp_);
    const int unit = lrg_uniform(unit_);
    const LrgAsyncArgs &A = LRG_ASYNC_KARGS().A;
    const LrgGemvArgs &g = A.gemv;
    const int P = g.P, kq = P >> 3;
    const int upz = g.C / LRG_GEMV_UNIT_COLS;
    const int z = unit / upz, col0 = (unit - z * upz) * LRG_GEMV_UNIT_COLS;
    float *wl = lrg_async_smem;                                // [P][32] this unit's columns of head z's pooled kernel
    {
        const float *w = g.w[z] + col0;
        for (int i = threadIdx.x; i < P * (LRG_GEMV_UNIT_COLS / 4); i += LRG_FRONT_THREADS) {
            const int row = i >> 3, q = i & 7;
            *reinterpret_cast<float4 *>(wl + row * LRG_GEMV_UNIT_COLS + 4 * q) = *reinterpret_cast<const float4 *>(w + (long)row * g.ldw + 4 * q);
        }
    }
    const int ht = lrg_uniform((int)threadIdx.x >> 7);
    float *prow_lds = lrg_async_smem + P * LRG_GEMV_UNIT_COLS + ht * LRG_GEMV_UNIT2_TEAM_FLOATS(P);      // [P / 2] half of the slot's pooled row
    float *part = prow_lds + P / 2;                                                                 // [8][32] partial sums
    int *word = reinterpret_cast<int *>(part + 8 * LRG_GEMV_UNIT_COLS);                            // [0], [1] the task of even / odd rounds, [4] barrier counter
    int *ctl = reinterpret_cast<int *>(lrg_async_smem + P * LRG_GEMV_UNIT_COLS + 8 * LRG_GEMV_UNIT2_TEAM_FLOATS(P));      // [0] the unit's next ring entry
    if ((threadIdx.x & 127) == 0) { word[0] = 0; word[1] = 0; word[4] = 0; }
    if (threadIdx.x < 4) ctl[threadIdx.x] = 0;
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    LrgLdsPair pair;
    pair.cnt = &word[4]; pair.target = 0; pair.gave_up = &A.queue[LRG_AQ_ABORT];
    const int tid = (int)threadIdx.x & 127, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 31, h = lane >> 5;
    const float bias = g.bias[z] ? g.bias[z][col0 + c] : 0.f;
    const int32_t *ring = A.queue + LRG_AQ_RING + 2 * (A.qmask + 1);
    for (int round = 0;; round ^= 1) {
        long long t_task = 0;
        if (wave == 0) {
            int slot = -2;
            int i = 0;
            if (lane == 0) i = __hip_atomic_fetch_add(&ctl[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            i = __shfl(i, 0);
            const int32_t *e = ring + (i & A.gmask);
            const int tag = lrg_gemv_ring_tag(i, A.gmask);
            for (unsigned spin = 0; slot == -2; ++spin) {
                const int code = lrg_ld_coh(e);
                if ((code >> 20) == tag) { slot = code & 0xFFFFF; break; }
                if ((spin & 7) == 7) {
                    if (lrg_ld_coh(&A.queue[LRG_AQ_FRONTS_DONE]) >= A.n_front || lrg_ld_coh(&A.queue[LRG_AQ_ABORT])) slot = -1;
                    else if ((spin & 1023) == 1023 && wall_clock64() - t_launch > A.abort_ticks) { lrg_st_coh(&A.queue[LRG_AQ_ABORT], 4); slot = -1; }
                }
                if (slot == -2) __builtin_amdgcn_s_sleep(2);
            }
            if (lane == 0) word[round] = slot;
        }
        pair.sync();
        const int entry = word[round];
        if (entry < 0) return;
        const int slot = entry & 0xFFF;
        if (LRG_DBG(A)) t_task = wall_clock64();
        // the slot's pooled row: ONE trip -- every thread of the pair takes 16 bytes of either half (four K ranges each) -- and half a row at a time in LDS: eight
        // staged HALF rows are what fits beside the slice.  Ranges 2 wave + h (first half) and 4 + 2 wave + h (second): each a chain of kq FMAs.
        const float4 ph0 = lrg_ld_coh4(g.pooled + (long)slot * P, (unsigned)tid * 16u), ph1 = lrg_ld_coh4(g.pooled + (long)slot * P, (unsigned)(128 + tid) * 16u);
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            if (pass) pair.sync();                                   // (everybody is done with the first half)
            *reinterpret_cast<float4 *>(prow_lds + 4 * tid) = pass ? ph1 : ph0;
            pair.sync();
            const int rl = 2 * wave + h, r = 4 * pass + rl;
            const float *w = wl + (r * kq) * LRG_GEMV_UNIT_COLS + c;
            const float *p = prow_lds + rl * kq;
            float acc = 0.f;
            for (int kb = 0; kb < kq; kb += 16) {
                float wv[16];
                float4 pv[4];
#pragma unroll
                for (int u = 0; u < 16; ++u) wv[u] = w[(kb + u) * LRG_GEMV_UNIT_COLS];
#pragma unroll
                for (int u = 0; u < 4; ++u) pv[u] = *reinterpret_cast<const float4 *>(p + kb + 4 * u);
                const float pk[16] = {pv[0].x, pv[0].y, pv[0].z, pv[0].w, pv[1].x, pv[1].y, pv[1].z, pv[1].w,
                                      pv[2].x, pv[2].y, pv[2].z, pv[2].w, pv[3].x, pv[3].y, pv[3].z, pv[3].w};
#pragma unroll
                for (int uu = 0; uu < 16; ++uu) {
                    const int u = (uu & 8) | ((uu & 1) << 2) | ((uu >> 1) & 3);      // k = 8g + 0, 4, 1, 5, 2, 6, 3, 7 (lrg_async_gemv)
                    acc = fmaf(pk[u], wv[u], acc);
                }
            }
            part[r * LRG_GEMV_UNIT_COLS + c] = acc;
        }
        pair.sync();
        // the sums and the arrival by the second wavefront: the first is back at the ring while these stores drain
        if (wave == 1) {
            float sum = part[lane & (LRG_GEMV_UNIT_COLS - 1)];
#pragma unroll
            for (int q = 1; q < 8; ++q) sum += part[q * LRG_GEMV_UNIT_COLS + (lane & (LRG_GEMV_UNIT_COLS - 1))];
            sum += bias;
            const float v0 = __shfl(sum, 4 * (lane & 7)), v1 = __shfl(sum, 4 * (lane & 7) + 1), v2 = __shfl(sum, 4 * (lane & 7) + 2), v3 = __shfl(sum, 4 * (lane & 7) + 3);
            if (lane < LRG_GEMV_UNIT_COLS / 4) lrg_st_coh4(g.hb[z] + (long)slot * g.C + col0, (unsigned)lane * 16u, make_float4(v0, v1, v2, v3));
            lrg_drain_stores();
            if (lane == 0) {
                int32_t *sy = A.sync + (long)slot * LRG_ASYNC_SYNC_WORDS;
                if (LRG_DBG(A)) {
                    const int done = __hip_atomic_fetch_add(&sy[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
                    const long long now = wall_clock64();
                    lrg_dbg_add(A, 8 + 2 * LRG_TASK_GEMV, now - t_task); lrg_dbg_add(A, 9 + 2 * LRG_TASK_GEMV, 1);
                    if (done == lrg_ld_coh(&sy[5])) lrg_dbg_add(A, 3, (int)((unsigned)now - (unsigned)lrg_ld_coh(&sy[8])));
                } else {
                    __hip_atomic_fetch_add(&sy[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    }
}

// ---- a pooled-product unit with its slice in REGISTERS: rows streamed through LDS ----
// The two forms above sit under two ceilings that lie side by side: the tasks in flight (four or eight per unit, each ~3 us of latencies) and the LDS array of the
// unit's CU, which reads the whole 128 KB slice again for every task (~1 000 cycles) beside the pooled values (~500).  Here no weight is read from LDS per task and
// nothing that is a latency holds anything else up:
//   ENGINES   wavefronts 0 .. 7, one per K range.  Lane (column c = lane & 31, half h = lane >> 5) keeps the 64 weights of k-groups 8h .. 8h + 7 of its range in
//             registers for the whole launch.  A BEAT is 64 FMAs per lane: lanes 0 - 31 run the first half-chain of task t from zero while lanes 32 - 63 run the
//             second half-chain of task t - 1 on the accumulator handed across the lane halves -- two tasks in the pipe, no barrier.  When row t is not staged yet the
//             beat runs for the second half alone: a task in the pipe never waits for the next to arrive.  The pooled values come as 16-byte LDS reads whose address
//             is uniform per lane half (a broadcast): 8 wavefronts x 16 reads x 4 cycles = 512 LDS-array cycles a task, the partial sums and flags a few dozen more.
//   FETCHERS  wavefronts 8 .. 11.  Fetcher f takes the unit's ring positions f, f + 4, ...: waits for the FIFO slot to be free and the tagged entry to be there, loads
//             the row (or the maximum over the tile rows) into the slot and marks it ready.  Four entries' trips are in flight at once.
//   WRITERS   wavefronts 12 .. 15.  Writer q takes the tasks q, q + 4, ...: when all eight partial sums are in it adds them in order, adds the bias, frees the FIFO
//             slot, stores, drains and arrives, while the engines are already on the next tasks.
// The FIFO: LRG_GEMV_UNIT3_ROWS staged rows of 4 KB with their eight rows of partial sums and four words each -- `ready` (position + 1, by the fetcher), `done`
// (engines that have written their partial sum: 8 per turn of the FIFO, never reset), `freed` (position + 1, by the writer once it has read the sums) and the ring
// entry.  A position's slot is position % ROWS: the engines take the positions in ring order, as the teams' ticket does.
// Leaving: the front workgroups are done only when every evaluation is, and an evaluation needs every unit's arrival -- so whoever waits and sees that the fronts
// are done (or the abort word set) has nothing in flight, and every wavefront looks for itself; no wait depends on another wavefront's having seen it.
// Sums: per K range one chain over k = 8g + 0, 4, 1, 5, 2, 6, 3, 7 for g ascending (the two half-chains are one chain: the second starts from the first's sum),
// the eight partial sums in order, the bias last -- lrg_async_gemv_unit's bit for bit.  For P = 1024 and units of 32 columns only (the plan's gate: unit_regs).
#define LRG_GEMV_UNIT3_ROWS 16
#define LRG_GEMV_UNIT3_P 1024
#define LRG_GEMV_UNIT3_FLOATS (LRG_GEMV_UNIT3_ROWS * (LRG_GEMV_UNIT3_P + 8 * LRG_GEMV_UNIT_COLS + 8))

// one look at the launch's end from inside a wait (true: leave); the wall clock every `clock_every` looks (a power of two)
__device__ __forceinline__ bool lrg_unit3_leave(const LrgAsyncArgs &A, long long t_launch, unsigned look, unsigned clock_every) {
    if (lrg_ld_coh(&A.queue[LRG_AQ_FRONTS_DONE]) >= A.n_front || lrg_ld_coh(&A.queue[LRG_AQ_ABORT])) return true;
    if ((look & (clock_every - 1)) == clock_every - 1 && wall_clock64() - t_launch > A.abort_ticks) {
        lrg_st_coh(&A.queue[LRG_AQ_ABORT], 4);
        return true;
    }
    return false;
}
__device__ __forceinline__ int lrg_unit3_flag(const int *w) { return lrg_uniform(__hip_atomic_load(const_cast<int *>(w), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)); }

LRG_ASYNC_ROLE void lrg_async_gemv_unit3(lrg_kargs_ptr kp_, int unit_, long long t_launch) {
    const lrg_kargs_ptr kp = lrg_uniform(kp_);
    const int unit = lrg_uniform(unit_);
    const LrgAsyncArgs &A = LRG_ASYNC_KARGS().A;
    const LrgGemvArgs &g = A.gemv;
    constexpr int P = LRG_GEMV_UNIT3_P, NF = LRG_GEMV_UNIT3_ROWS, KR = P / 8;      // (KR: a K range, 128)
    const int upz = g.C / LRG_GEMV_UNIT_COLS;
    const int z = unit / upz, col0 = (unit - z * upz) * LRG_GEMV_UNIT_COLS;
    float *rows = lrg_async_smem;                                   // [NF][P] staged pooled rows
    float *part = rows + NF * P;                                    // [NF][8][32] partial sums
    int *ctl = reinterpret_cast<int *>(part + NF * 8 * LRG_GEMV_UNIT_COLS);
    int *ready = ctl, *done = ctl + NF, *freed = ctl + 2 * NF, *ent = ctl + 3 * NF, *stamp = ctl + 4 * NF;      // (stamp: two words per slot, debug builds)
    const int wave = lrg_uniform((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    const int c = lane & 31, h = lane >> 5;
    if (threadIdx.x < 8 * NF) ctl[threadIdx.x] = 0;
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                                   // the flags are zero; from here on every wavefront goes its own way

    if (wave < 8) {
        // ---- an engine: K range `wave` ----
        float w[64];                                                // the slice, once per launch: this lane's 64 weights, in k order
        {
            const float *wp = g.w[z] + col0 + c + (long)(wave * KR + h * 64) * g.ldw;
#pragma unroll
            for (int j = 0; j < 64; ++j) w[j] = wp[(long)j * g.ldw];
        }
        int n = 0;                                                  // the next ring position to start
        bool pending = false;                                       // position n - 1 has its first half-chain and waits for the second
        float prev = 0.f;
        for (;;) {
            const int s_new = n & (NF - 1), s_old = (n - 1) & (NF - 1);
            bool have = false;
            if (pending) {
                have = lrg_unit3_flag(&ready[s_new]) == n + 1;      // (one look: the task in the pipe goes on either way)
            } else {
                for (unsigned spin = 0;; ++spin) {
                    if (lrg_unit3_flag(&ready[s_new]) == n + 1) { have = true; break; }
                    if ((spin & 63u) == 63u && lrg_unit3_leave(A, t_launch, spin >> 6, 64u)) return;
                    __builtin_amdgcn_s_sleep(1);
                }
            }
            asm volatile("" ::: "memory");
            // (a half with no task of its own reads the other's row and its sum is dropped)
            const float *p = rows + ((h || !have) ? s_old : s_new) * P + wave * KR + h * 64;
            float acc = __shfl(prev, c);
            acc = h ? acc : 0.f;
            // 64 weights and 64 pooled values do not fit 128 registers: the values come sixteen at a time, two reads of sixteen ahead of the FMAs
            // (the fences keep the compiler from taking all sixteen 16-byte reads to the top, which spills weights inside this loop)
            float4 pa[4], pb[4];
            auto read16 = [&](float4 (&pv)[4], int kb) {
#pragma unroll
                for (int u = 0; u < 4; ++u) pv[u] = *reinterpret_cast<const float4 *>(p + kb + 4 * u);
            };
            auto fma16 = [&](const float4 (&pv)[4], int kb) {
                const float pk[16] = {pv[0].x, pv[0].y, pv[0].z, pv[0].w, pv[1].x, pv[1].y, pv[1].z, pv[1].w,
                                      pv[2].x, pv[2].y, pv[2].z, pv[2].w, pv[3].x, pv[3].y, pv[3].z, pv[3].w};
#pragma unroll
                for (int uu = 0; uu < 16; ++uu) {
                    const int u = (uu & 8) | ((uu & 1) << 2) | ((uu >> 1) & 3);      // k = 8g + 0, 4, 1, 5, 2, 6, 3, 7 (lrg_async_gemv)
                    acc = fmaf(pk[u], w[kb + u], acc);
                }
            };
            // (the running sum goes THROUGH the fence: the FMAs before it stay before it, and no LDS read crosses it)
            auto fence = [&] { asm volatile("" : "+v"(acc) : : "memory"); };
            read16(pa, 0); read16(pb, 16);
            fence();
            fma16(pa, 0);
            fence();
            read16(pa, 32);
            fma16(pb, 16);
            fence();
            read16(pb, 48);
            fma16(pa, 32); fma16(pb, 48);
            if (pending) {
                if (h) part[(s_old * 8 + wave) * LRG_GEMV_UNIT_COLS + c] = acc;
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (lane == 0) __hip_atomic_fetch_add(&done[s_old], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            prev = acc;
            pending = have;
            n += have ? 1 : 0;
        }
    } else if (wave < 12) {
        // ---- a fetcher: ring positions wave - 8, + 4, ... ----
        const int32_t *ring = A.queue + LRG_AQ_RING + 2 * (A.qmask + 1);
        int entry = 0;
        bool looked = false;                                        // `entry` is this position's, seen by the look that rode along with the last row's trip
        for (int n = wave - 8;; n += 4) {
            const int s = n & (NF - 1);
            if (n >= NF)      // the slot's last task has been summed up
                for (unsigned spin = 0; lrg_unit3_flag(&freed[s]) < n - NF + 1; ++spin) {
                    if ((spin & 63u) == 63u && lrg_unit3_leave(A, t_launch, spin >> 6, 64u)) return;
                    __builtin_amdgcn_s_sleep(1);
                }
            const int32_t *e = ring + (n & A.gmask);
            const int tag = lrg_gemv_ring_tag(n, A.gmask);
            for (unsigned spin = 0; !looked; ++spin) {
                entry = lrg_uniform(lrg_ld_coh(e));
                if ((entry >> 20) == tag) break;
                if ((spin & 7u) == 7u && lrg_unit3_leave(A, t_launch, spin >> 3, 128u)) return;
                __builtin_amdgcn_s_sleep(2);
            }
            const int slot = entry & 0xFFF;                         // (units serve at most LRG_GEMV_UNIT_MAX_SLOTS = 2048 slots)
            if (LRG_DBG(A) && lane == 0) { const long long t = wall_clock64(); stamp[2 * s] = (int)t; stamp[2 * s + 1] = (int)(t >> 32); }
            float *dst = rows + s * P;
            // one look at this fetcher's NEXT position travels with the row's loads: with the ring full a fetcher's turn is one trip, not two
            const int ahead = lrg_ld_coh(ring + ((n + 4) & A.gmask));
            if (A.pool_rows) {
                // the maximum over the slot's branch tiles' rows, taken on the way into LDS (the values are >= 0: their order is that of their bit patterns).
                // A lane owns four 16-byte pieces, two per side, and has four tiles' loads of each in flight (past a side's last tile: that tile again).
                const int nt_in = ((entry >> 16) & 15) + 1, nt_nb = ((entry >> 12) & 15) + 1;
                const float *src = A.pool_rows + (long)slot * A.pool_rows_stride;
                int4 m[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) m[q] = make_int4(0, 0, 0, 0);
                for (int t0 = 0; t0 < max(nt_in, nt_nb); t0 += 4) {
                    float4 v[4][4];
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const int tile = min(t0 + t, (q >= 2 ? nt_nb : nt_in) - 1);
                            v[q][t] = lrg_ld_coh4(src + (q >= 2 ? 16 * (P >> 1) : 0), (unsigned)(tile * (P >> 1) + 4 * (lane + 64 * (q & 1))) * 4u);
                        }
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            m[q].x = max(m[q].x, __float_as_int(v[q][t].x)); m[q].y = max(m[q].y, __float_as_int(v[q][t].y));
                            m[q].z = max(m[q].z, __float_as_int(v[q][t].z)); m[q].w = max(m[q].w, __float_as_int(v[q][t].w));
                        }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) *reinterpret_cast<int4 *>(dst + 4 * (lane + 64 * q)) = m[q];
            } else {   // the slot's pooled row: four 16-byte loads per lane, one trip
                const float *src = g.pooled + (long)slot * P;
                float4 v[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = lrg_ld_coh4(src, (unsigned)(lane + 64 * q) * 16u);
#pragma unroll
                for (int q = 0; q < 4; ++q) *reinterpret_cast<float4 *>(dst + 4 * (lane + 64 * q)) = v[q];
            }
            if (lane == 0) ent[s] = entry;
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");      // the row is in LDS before it is called ready
            if (lane == 0) __hip_atomic_store(&ready[s], n + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            entry = lrg_uniform(ahead);
            looked = (entry >> 20) == lrg_gemv_ring_tag(n + 4, A.gmask);
        }
    } else {
        // ---- a writer: tasks wave - 12, + 4, ... ----
        const float bias = g.bias[z] ? g.bias[z][col0 + c] : 0.f;
        for (int n = wave - 12;; n += 4) {
            const int s = n & (NF - 1), want = 8 * (n / NF + 1);
            for (unsigned spin = 0; lrg_unit3_flag(&done[s]) < want; ++spin) {
                if ((spin & 63u) == 63u && lrg_unit3_leave(A, t_launch, spin >> 6, 64u)) return;
                __builtin_amdgcn_s_sleep(1);
            }
            asm volatile("" ::: "memory");
            const int slot = lrg_uniform(ent[s]) & 0xFFF;
            long long t_task = 0;
            if (LRG_DBG(A)) t_task = ((long long)stamp[2 * s + 1] << 32) | (unsigned)stamp[2 * s];
            float sum = part[s * 8 * LRG_GEMV_UNIT_COLS + c];
#pragma unroll
            for (int q = 1; q < 8; ++q) sum += part[(s * 8 + q) * LRG_GEMV_UNIT_COLS + c];
            sum += bias;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the sums are read: the FIFO slot may be staged again
            if (lane == 0) __hip_atomic_store(&freed[s], n + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const float v0 = __shfl(sum, 4 * (lane & 7)), v1 = __shfl(sum, 4 * (lane & 7) + 1), v2 = __shfl(sum, 4 * (lane & 7) + 2), v3 = __shfl(sum, 4 * (lane & 7) + 3);
            if (lane < LRG_GEMV_UNIT_COLS / 4) lrg_st_coh4(g.hb[z] + (long)slot * g.C + col0, (unsigned)lane * 16u, make_float4(v0, v1, v2, v3));
            lrg_drain_stores();
            if (lane == 0) {
                int32_t *sy = A.sync + (long)slot * LRG_ASYNC_SYNC_WORDS;
                if (LRG_DBG(A)) {
                    const int arrived = __hip_atomic_fetch_add(&sy[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
                    const long long now = wall_clock64();
                    lrg_dbg_add(A, 8 + 2 * LRG_TASK_GEMV, now - t_task); lrg_dbg_add(A, 9 + 2 * LRG_TASK_GEMV, 1);
                    if (arrived == lrg_ld_coh(&sy[5])) lrg_dbg_add(A, 3, (int)((unsigned)now - (unsigned)lrg_ld_coh(&sy[8])));
                } else {
                    __hip_atomic_fetch_add(&sy[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    }
}
