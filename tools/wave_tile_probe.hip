// Probe for csrc/lrg_wave_tile.inl (round 6): one wavefront = one 32-row branch tile with the activations in registers.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I learn_region_grow_amd/csrc tools/wave_tile_probe.hip -o gpurun_out/wave_tile_probe
// Checks conv[1] and the pooled maxima bit for bit against a host evaluation in the MFMA formulation's summation order (per output a chain of FMAs over
// k = 8g + 0, 4, 1, 5, 2, 6, 3, 7, then bias, then ReLU: lrg_fused_tile.inl), and times a task with 1 .. 16 wavefronts per CU on 1 / 64 / 200 CUs.
// `wave_tile_probe pairs`: the register branch tile on the teams of a 512-thread workgroup, as the free-running worker kernel runs it (pairs_kernel below).
// `wave_tile_probe roles`: head and branch teams of such a workgroup by the role of their CU -- who shares the SIMDs with whom (roles_kernel below).
// `wave_tile_probe units`: the three forms of the pooled-product units (csrc/lrg_async_units.inl), each alone on hand-made rows and ring entries (units_kernel below).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
extern __shared__ __attribute__((aligned(16))) float lrg_async_smem[];
#include "lrg_wave_tile.inl"
// (mode `units`: the pooled-product units as lrg_async.inl includes them -- the few words it defines before that, said again here)
#include "lrg_async_plan.h"
#define LRG_FRONT_THREADS 1024
#define LRG_ASYNC_SYNC_WORDS 16
#define LRG_TASK_GEMV 2
#define LRG_ASYNC_DEBUG 0
#define LRG_DBG(A) (LRG_ASYNC_DEBUG && (A).dbg)
__device__ __forceinline__ void lrg_dbg_add(const LrgAsyncArgs &A, int i, long long v) { if (LRG_DBG(A)) atomicAdd(&A.dbg[i], (unsigned long long)v); }
__device__ __forceinline__ void lrg_drain_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
#include "lrg_async_units.inl"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(1); } } while (0)

struct Args {
    const float *w[5];       // packed images (lrg_pack_weights layout)
    const float *b[5];
    const float *x, *center;
    float *conv1, *h3, *pool;     // pool: [slots][512]
    long long *cycles;       // [workgroups][16]
    int n_tiles, rows_per_slot, iters, waves, stage;
    LrgFusedProb head;       // stage 3: the register head tile's problem (x = conv[1] rows, L[0] / L[1], fw / fb / fout)
};

// stage 0: PREFIX tasks (layers 0 - 3 -> conv[1], layer-3 rows); stage 1: POOL tasks (workgroup & 1 = the half of the pooled layer's columns it holds)
__global__ __launch_bounds__(512) void probe_kernel(Args a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = blockIdx.x & 1;
    if (a.stage == 0) {
        const int sizes[4] = {1024, 4096, 4096, 8192}, offs[4] = {LRG_WA_W0, LRG_WA_W1, LRG_WA_W2, LRG_WA_W3};
        const int bs[4] = {64, 64, 64, 128}, bo[4] = {LRG_WA_B0, LRG_WA_B1, LRG_WA_B2, LRG_WA_B3};
        for (int side = 0; side < 2; ++side)      // (the probe has one branch: both halves of the LDS hold it, the odd tiles use the second copy)
            for (int l = 0; l < 4; ++l) {
                for (int i = tid; i < sizes[l] / 4; i += 512) reinterpret_cast<float4 *>(lrg_async_smem + side * LRG_WA_SIDE + offs[l])[i] = reinterpret_cast<const float4 *>(a.w[l])[i];
                for (int i = tid; i < bs[l]; i += 512) lrg_async_smem[side * LRG_WA_SIDE + bo[l] + i] = a.b[l][i];
            }
    } else {
        for (int qq = 0; qq < 2; ++qq) {
            const int q = 2 * half + qq;
            for (int i = tid; i < 4096; i += 512) reinterpret_cast<float4 *>(lrg_async_smem + qq * LRG_WP_QUARTER + LRG_WP_W4)[i] = reinterpret_cast<const float4 *>(a.w[4] + (long)q * 16384)[i];
            for (int i = tid; i < 128; i += 512) lrg_async_smem[qq * LRG_WP_QUARTER + LRG_WP_B4 + i] = a.b[4][q * 128 + i];
        }
    }
    if (a.stage == 3) {
        // REGISTER HEAD TILE: one team of four wavefronts per tile
        LrgWgTeam team;
        struct { __device__ void operator()() const {} } nowait;
        const long long t0 = (long long)__builtin_readcyclecounter();
        for (int it = 0; it < a.iters; ++it) {
            const int tile = (blockIdx.x + it * 7) % a.n_tiles;
            const long r0 = (long)tile * 32;
            lrg_team_head_tile_reg(a.head, r0, (int)(r0 / a.rows_per_slot), 0, team, nowait, wave, lane);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
        const long long t1 = (long long)__builtin_readcyclecounter();
        if (lane == 0) a.cycles[blockIdx.x * 16 + wave] = t1 - t0;
        return;
    }
    if (a.stage == 2) {
        // REGISTER TILE: the workgroup = one team of four wavefronts per tile; both halves of the kernels' LDS hold the probe's one branch
        const int sizes[3] = {1024, 4096, 4096}, offs[3] = {LRG_RT_W0, LRG_RT_W1, LRG_RT_W2};
        const int bs[5] = {64, 64, 64, 128, 512}, bo[5] = {LRG_RT_B0, LRG_RT_B1, LRG_RT_B2, LRG_RT_B3, LRG_RT_B4};
        for (int side = 0; side < 2; ++side) {
            for (int l = 0; l < 3; ++l)
                for (int i = tid; i < sizes[l] / 4; i += blockDim.x) reinterpret_cast<float4 *>(lrg_async_smem + side * LRG_RT_SIDE + offs[l])[i] = reinterpret_cast<const float4 *>(a.w[l])[i];
            for (int l = 0; l < 5; ++l)
                for (int i = tid; i < bs[l]; i += blockDim.x) lrg_async_smem[side * LRG_RT_SIDE + bo[l] + i] = a.b[l][i];
        }
        int *pair_cnt = reinterpret_cast<int *>(lrg_async_smem + LRG_RT_WEIGHT_FLOATS + LRG_RT_PAIR_CNT);
        if (tid < 2) pair_cnt[tid] = 0;
        __syncthreads();
        LrgWgTeam team;
        const int wn = __builtin_amdgcn_readfirstlane(wave);
        LrgLdsPair pair;
        pair.cnt = pair_cnt + (wn >> 1); pair.target = 0; pair.gave_up = nullptr;
        const long long t0 = (long long)__builtin_readcyclecounter();
        for (int it = 0; it < a.iters; ++it) {
            const int tile = (blockIdx.x + it * 7) % a.n_tiles;
            const long r0 = (long)tile * 32;
            lrg_team_branch_tile_reg<1>(a.x, a.center, a.conv1, a.pool + (r0 / a.rows_per_slot) * 512, a.w[3], a.w[4], r0, (int)(r0 / a.rows_per_slot), (tile & 1) * LRG_RT_SIDE,
                                     LRG_RT_WEIGHT_FLOATS, team, pair, wn, lane);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();                                  // (as the task does before its arrival; the exchange buffer is free again)
        }
        const long long t1 = (long long)__builtin_readcyclecounter();
        if (lane == 0) a.cycles[blockIdx.x * 16 + wave] = t1 - t0;
        return;
    }
    __syncthreads();
    if (wave >= a.waves) return;
    const long long t0 = (long long)__builtin_readcyclecounter();
    for (int it = 0; it < a.iters; ++it) {
        const int job = (blockIdx.x >> 1) * a.waves + wave + it * 7;
        if (a.stage == 0) {
            const int tile = (2 * job + half) % a.n_tiles;
            const long r0 = (long)tile * 32;
            lrg_wave_prefix_tile(a.x, a.center, a.conv1, a.h3, r0, (int)(r0 / a.rows_per_slot), (tile & 1) * LRG_WA_SIDE, lane);
        } else {
            const int tile = (job >> 1) % a.n_tiles, q = 2 * half + (job & 1);
            const long r0 = (long)tile * 32;
            lrg_wave_pool_tile(a.h3, a.pool + (r0 / a.rows_per_slot) * 512, r0, q, (q & 1) * LRG_WP_QUARTER, 0, 2, lane);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const long long t1 = (long long)__builtin_readcyclecounter();
    if (lane == 0) a.cycles[blockIdx.x * 16 + wave] = t1 - t0;
}

static void pack(const std::vector<float> &w, int K, int N, std::vector<float> &out) {
    const int ng = (K + 7) / 8, ncb = (N + 31) / 32;
    out.assign((size_t)ncb * ng * 64 * 4, 0.f);
    for (int cb = 0; cb < ncb; ++cb)
        for (int g = 0; g < ng; ++g)
            for (int lane = 0; lane < 64; ++lane)
                for (int s = 0; s < 4; ++s) {
                    const int col = 32 * cb + (lane & 31), k = 8 * g + 4 * (lane >> 5) + s;
                    out[(((size_t)cb * ng + g) * 64 + lane) * 4 + s] = (k < K && col < N) ? w[(size_t)k * N + col] : 0.f;
                }
}

static void layer_ref(const std::vector<float> &in, int rows, int K, const std::vector<float> &w, const std::vector<float> &b, int N, std::vector<float> &out) {
    const int ng = (K + 7) / 8;
    out.assign((size_t)rows * N, 0.f);
    for (int n = 0; n < rows; ++n)
        for (int c = 0; c < N; ++c) {
            float acc = 0.f;
            for (int g = 0; g < ng; ++g)
                for (int s = 0; s < 4; ++s)
                    for (int h = 0; h < 2; ++h) {
                        const int k = 8 * g + 4 * h + s;
                        const float xv = k < K ? in[(size_t)n * K + k] : 0.f, wv = k < K ? w[(size_t)k * N + c] : 0.f;
                        acc = fmaf(wv, xv, acc);
                    }
            out[(size_t)n * N + c] = fmaxf(acc + b[c], 0.f);
        }
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------------------
// `wave_tile_probe pairs`: the register branch tile as the free-running worker kernel runs it (tests/test_gpu_branch_tile_pairs.py) -- teams of a 512-thread
// workgroup meeting at LDS counters (LrgLdsTeam, LrgLdsPair), two branches with kernels of their own at the two `ws` offsets, one or two parts per tile, tiles back to
// back, a second branch team or a head team on the workgroup's other half.  The LDS is the worker's: [kernels of both sides][team 0: control words, exchange
// buffer][team 1: control words, a head tile's buffers].
#define P_CTL 24
#define P_TEAM0 (P_CTL + LRG_RT_XCH_FLOATS)
#define P_TEAM1 (P_CTL + LRG_RH_FLOATS)
#define P_LDS_FLOATS (LRG_RT_WEIGHT_FLOATS + P_TEAM0 + P_TEAM1)
struct PArgs {
    const float *w[2][5], *b[2][5];      // per side: packed images, biases
    const float *x, *center;
    float *conv1, *h3, *pool;            // h3: nullable (timing)
    long long *cycles;                   // [workgroups][2]
    int tile0, tile_mod, tiles_per_team, tiles_per_slot, nparts, iters, head_beside;      // tile = tile0 + (its number in the launch) % tile_mod
    LrgFusedProb head;
    int kind[2], background;             // roles_kernel: what team 0 / 1 runs (0: absent, 1: branch tiles, 2: head tiles); the team that runs until the other is through (-1: none)
};
__global__ __launch_bounds__(512) void pairs_kernel(PArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, nteams = (int)blockDim.x >> 8;
    // (wave-uniform, and known to the compiler as such: the tile's kernel pointers depend on them -- a buffer load whose descriptor is not uniform becomes a loop)
    const int t = __builtin_amdgcn_readfirstlane(tid >> 8), wn = __builtin_amdgcn_readfirstlane((tid >> 6) & 3);
    {
        const int sizes[3] = {1024, 4096, 4096}, offs[3] = {LRG_RT_W0, LRG_RT_W1, LRG_RT_W2};
        const int bs[5] = {64, 64, 64, 128, 512}, bo[5] = {LRG_RT_B0, LRG_RT_B1, LRG_RT_B2, LRG_RT_B3, LRG_RT_B4};
        for (int side = 0; side < 2; ++side) {
            for (int l = 0; l < 3; ++l)
                for (int i = tid; i < sizes[l] / 4; i += blockDim.x) reinterpret_cast<float4 *>(lrg_async_smem + side * LRG_RT_SIDE + offs[l])[i] = reinterpret_cast<const float4 *>(a.w[side][l])[i];
            for (int l = 0; l < 5; ++l)
                for (int i = tid; i < bs[l]; i += blockDim.x) lrg_async_smem[side * LRG_RT_SIDE + bo[l] + i] = a.b[side][l][i];
        }
    }
    const int region = LRG_RT_WEIGHT_FLOATS + t * P_TEAM0, xch = region + P_CTL;
    int *word = reinterpret_cast<int *>(lrg_async_smem + region);      // [0] the head team's 'go on', [4] the team's counter, [6] team 0: 'done'
    int *pair_cnt = reinterpret_cast<int *>(lrg_async_smem + xch + LRG_RT_PAIR_CNT);
    if ((tid & 255) == 0) { word[0] = 1; word[4] = 0; word[6] = 0; }
    if ((tid & 255) < 2) pair_cnt[tid & 255] = 0;
    __syncthreads();
    LrgLdsTeam team;
    team.cnt = &word[4]; team.target = 0; team.base = t * 256; team.gave_up = nullptr;
    if (a.head_beside && t == 1) {
        // head tiles until the branch team is through (bounded)
        volatile int *done = reinterpret_cast<volatile int *>(lrg_async_smem + LRG_RT_WEIGHT_FLOATS) + 6;
        struct { __device__ void operator()() const {} } nowait;
        for (int it = 0; it < 16 * a.iters * a.tiles_per_team; ++it) {
            if (tid == 256) word[0] = !*done;
            team.sync();
            const int go = word[0];
            if (!go) break;
            lrg_team_head_tile_reg(a.head, (long)(it % a.tiles_per_team) * 32, 0, xch, team, nowait, wn, lane);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            team.sync();
        }
        return;
    }
    LrgLdsPair pair;
    pair.cnt = pair_cnt + (wn >> 1); pair.target = 0; pair.gave_up = nullptr;
    const int li = lane & 31, lh = lane >> 5;
    const long long t0 = (long long)__builtin_readcyclecounter();
    for (int it = 0; it < a.iters * a.tiles_per_team; ++it) {
        const int tile = a.tile0 + (((int)blockIdx.x * nteams + t) * a.tiles_per_team + it % a.tiles_per_team) % a.tile_mod;
        const int slot = tile / a.tiles_per_slot, side = slot & 1;
        const long r0 = (long)tile * 32;
        for (int part = 0; part < a.nparts; ++part) {
            if (a.nparts == 2)
                lrg_team_branch_tile_reg<2>(a.x, a.center, a.conv1, a.pool + (long)slot * 512, a.w[side][3], a.w[side][4], r0, slot, side * LRG_RT_SIDE, xch, team, pair, wn, lane, part);
            else
                lrg_team_branch_tile_reg<1>(a.x, a.center, a.conv1, a.pool + (long)slot * 512, a.w[side][3], a.w[side][4], r0, slot, side * LRG_RT_SIDE, xch, team, pair, wn, lane, 0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            team.sync();                                      // (as the task does before its arrival)
            if (a.h3 && part == 0) {
                // layer 3's rows as the tile left them in the exchange buffer: wavefront wn copies block wn
                for (int j = 0; j < 4; ++j)
                    *reinterpret_cast<float4 *>(a.h3 + (r0 + li) * 128 + 32 * wn + 8 * j + 4 * lh) = lrg_wb_lds4(xch + lrg_rt_xch_l3(wn, j, lane));
            }
            team.sync();                                      // (the next task's first meeting)
        }
    }
    const long long t1 = (long long)__builtin_readcyclecounter();
    if ((tid & 255) == 0) {
        a.cycles[blockIdx.x * 2 + t] = t1 - t0;
        if (t == 0) word[6] = 1;
    }
}

// `wave_tile_probe roles`: the teams of a register-tile CU by role (csrc/lrg_async_plan.h, lrg_rt_role; tests/test_gpu_cu_roles.py) -- a head team alone, beside a
// second head team, beside a branch team; a branch team with team 1 absent.  The LDS is the worker's, and a CU whose team 0 runs head tiles (HEAD2) holds no branch
// kernels: team 0's head region lies in their place, team 1's where it always is.  A team runs iters x tiles_per_team tiles and is timed, or (`background`) runs
// until the other team is through.  Head tile h = 64 t + (its number) % 64 is slot h's: the pooled product (layer 0's bias) is a row per slot.
__global__ __launch_bounds__(512) void roles_kernel(PArgs a) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int t = __builtin_amdgcn_readfirstlane(tid >> 8), wn = __builtin_amdgcn_readfirstlane((tid >> 6) & 3);
    const bool head2 = a.kind[0] == 2;
    if (a.kind[0] == 1 || a.kind[1] == 1) {
        const int sizes[3] = {1024, 4096, 4096}, offs[3] = {LRG_RT_W0, LRG_RT_W1, LRG_RT_W2};
        const int bs[5] = {64, 64, 64, 128, 512}, bo[5] = {LRG_RT_B0, LRG_RT_B1, LRG_RT_B2, LRG_RT_B3, LRG_RT_B4};
        for (int side = 0; side < 2; ++side) {
            for (int l = 0; l < 3; ++l)
                for (int i = tid; i < sizes[l] / 4; i += blockDim.x) reinterpret_cast<float4 *>(lrg_async_smem + side * LRG_RT_SIDE + offs[l])[i] = reinterpret_cast<const float4 *>(a.w[side][l])[i];
            for (int l = 0; l < 5; ++l)
                for (int i = tid; i < bs[l]; i += blockDim.x) lrg_async_smem[side * LRG_RT_SIDE + bo[l] + i] = a.b[side][l][i];
        }
    }
    const int region0 = head2 ? 0 : LRG_RT_WEIGHT_FLOATS, region1 = LRG_RT_WEIGHT_FLOATS + P_TEAM0;
    const int region = t ? region1 : region0, xch = region + P_CTL;
    int *word = reinterpret_cast<int *>(lrg_async_smem + region);      // [0] a background team's 'go on', [4] the team's counter, [6] 'done'
    const int kind = a.kind[t];
    if ((tid & 255) == 0) { word[0] = 1; word[4] = 0; word[6] = 0; }
    if (kind == 1 && (tid & 255) < 2) reinterpret_cast<int *>(lrg_async_smem + xch + LRG_RT_PAIR_CNT)[tid & 255] = 0;
    __syncthreads();
    if (!kind) return;
    LrgLdsTeam team;
    team.cnt = &word[4]; team.target = 0; team.base = t * 256; team.gave_up = nullptr;
    LrgLdsPair pair;
    pair.cnt = reinterpret_cast<int *>(lrg_async_smem + xch + LRG_RT_PAIR_CNT) + (wn >> 1); pair.target = 0; pair.gave_up = nullptr;
    const bool background = a.background == t;
    volatile int *done = reinterpret_cast<volatile int *>(lrg_async_smem + (t ? region0 : region1)) + 6;
    struct { __device__ void operator()() const {} } nowait;
    const int n = (background ? 16 : 1) * a.iters * a.tiles_per_team;      // (bounded)
    const long long t0 = (long long)__builtin_readcyclecounter();
    for (int it = 0; it < n; ++it) {
        if (background) {
            if ((tid & 255) == 0) word[0] = !*done;
            team.sync();
            const int go = word[0];
            if (!go) break;
        }
        if (kind == 2) {
            const int h = t * a.tiles_per_team + it % a.tiles_per_team;
            lrg_team_head_tile_reg(a.head, (long)h * 32, h, xch, team, nowait, wn, lane);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            team.sync();                                      // (as the task does before its arrival)
        } else {
            const int tile = a.tile0 + (((int)blockIdx.x * 2 + t) * a.tiles_per_team + it % a.tiles_per_team) % a.tile_mod;
            const int slot = tile / a.tiles_per_slot, side = slot & 1;
            lrg_team_branch_tile_reg<1>(a.x, a.center, a.conv1, a.pool + (long)slot * 512, a.w[side][3], a.w[side][4], (long)tile * 32, slot, side * LRG_RT_SIDE, xch, team, pair, wn, lane, 0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            team.sync();
            team.sync();                                      // (the next task's first meeting, as in pairs_kernel)
        }
    }
    const long long t1 = (long long)__builtin_readcyclecounter();
    if ((tid & 255) == 0 && !background) {
        a.cycles[blockIdx.x * 2 + t] = t1 - t0;
        word[6] = 1;
    }
}

// the register head tile's host chain: the MFMA chain per layer (layer 0's bias is the slot's pooled product, then a zero layer bias), then lrg_fused_tile's last
// layer (eight partial chains over k = 4q + 32m + i, a butterfly over q)
static void head_ref(const std::vector<float> &cin, int rows, int rows_per_slot, const std::vector<float> &hw0, const std::vector<float> &hbv, const std::vector<float> &hw1,
                     const std::vector<float> &hbias1, const std::vector<float> &fw, const std::vector<float> &fb, std::vector<float> &lref) {
    std::vector<float> g0(256), g1h(128);
    lref.assign((size_t)rows * 2, 0.f);
    for (int n = 0; n < rows; ++n) {
        for (int c = 0; c < 256; ++c) {
            float acc = 0.f;
            for (int g = 0; g < 8; ++g) for (int s2 = 0; s2 < 4; ++s2) for (int hh = 0; hh < 2; ++hh) { const int k = 8 * g + 4 * hh + s2; acc = fmaf(hw0[(size_t)k * 256 + c], cin[(size_t)n * 64 + k], acc); }
            g0[c] = fmaxf((acc + hbv[(size_t)(n / rows_per_slot) * 256 + c]) + 0.f, 0.f);
        }
        for (int c = 0; c < 128; ++c) {
            float acc = 0.f;
            for (int g = 0; g < 32; ++g) for (int s2 = 0; s2 < 4; ++s2) for (int hh = 0; hh < 2; ++hh) { const int k = 8 * g + 4 * hh + s2; acc = fmaf(hw1[(size_t)k * 128 + c], g0[k], acc); }
            g1h[c] = fmaxf(acc + hbias1[c], 0.f);
        }
        float part[8][2];
        for (int q = 0; q < 8; ++q) {
            float s0 = 0.f, s1 = 0.f;
            for (int k = 4 * q; k < 128; k += 32)
                for (int i = 0; i < 4; ++i) { s0 = fmaf(g1h[k + i], fw[2 * (k + i)], s0); s1 = fmaf(g1h[k + i], fw[2 * (k + i) + 1], s1); }
            part[q][0] = s0; part[q][1] = s1;
        }
        for (int o = 0; o < 2; ++o) {
            const float t01 = part[0][o] + part[1][o], t23 = part[2][o] + part[3][o], t45 = part[4][o] + part[5][o], t67 = part[6][o] + part[7][o];
            lref[(size_t)n * 2 + o] = ((t01 + t23) + (t45 + t67)) + fb[o];
        }
    }
}

// one layer in the MFMA formulation's order; pre (nullable): the value before the ReLU
static void layer_ref2(const float *in, int rows, int K, const std::vector<float> &w, const std::vector<float> &b, int N, std::vector<float> &out, std::vector<float> *pre) {
    const int ng = (K + 7) / 8;
    out.assign((size_t)rows * N, 0.f);
    if (pre) pre->assign((size_t)rows * N, 0.f);
    for (int n = 0; n < rows; ++n)
        for (int c = 0; c < N; ++c) {
            float acc = 0.f;
            for (int g = 0; g < ng; ++g)
                for (int s = 0; s < 4; ++s)
                    for (int h = 0; h < 2; ++h) {
                        const int k = 8 * g + 4 * h + s;
                        const float xv = k < K ? in[(size_t)n * K + k] : 0.f, wv = k < K ? w[(size_t)k * N + c] : 0.f;
                        acc = fmaf(wv, xv, acc);
                    }
            if (pre) (*pre)[(size_t)n * N + c] = acc + b[c];
            out[(size_t)n * N + c] = fmaxf(acc + b[c], 0.f);
        }
}
static size_t differ(const std::vector<float> &g, const std::vector<float> &r, size_t first, size_t n) {
    size_t bad = 0;
    for (size_t i = first; i < first + n; ++i) bad += memcmp(&g[i], &r[i], 4) != 0;
    return bad;
}

static int pairs_main(bool roles) {
    const int n_tiles = 130, rows = n_tiles * 32, F = 13;      // tiles 0, 1: the single tiles and the two of one slot; 2 .. 129: the two teams' 64 each
    const int Ks[5] = {F, 64, 64, 64, 128}, Ns[5] = {64, 64, 64, 128, 512};
    srand(4711);
    auto rnd = []() { return (float)rand() / RAND_MAX * 2.f - 1.f; };
    std::vector<float> w[2][5], b[2][5], pk[2][5];
    for (int side = 0; side < 2; ++side)
        for (int l = 0; l < 5; ++l) {
            w[side][l].resize((size_t)Ks[l] * Ns[l]); b[side][l].resize(Ns[l]);
            const float sc = 1.5f / sqrtf((float)Ks[l]);
            for (auto &v : w[side][l]) v = rnd() * sc;
            for (auto &v : b[side][l]) v = rnd() * 0.1f;
            // every few columns of the pooled layer far below zero: no point's value is positive there, the pooled feature stays 0 (the path without an atomicMax)
            if (l == 4) for (int c = 0; c < 512; ++c) if (c % (side ? 5 : 7) == 3) b[side][l][c] = -1000.f;
            pack(w[side][l], Ks[l], Ns[l], pk[side][l]);
        }
    std::vector<float> x16((size_t)rows * 16, 0.f), cen((size_t)n_tiles * 16, 0.f);
    for (auto &v : cen) v = 0.f;
    for (int s = 0; s < n_tiles; ++s)
        for (int c = 0; c < F; ++c) cen[s * 16 + c] = (c < 2 || c >= 6) ? rnd() : 0.f;
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < F; ++c) x16[(size_t)r * 16 + c] = rnd() * 2.f;
    // host chain of tiles [t_lo, t_hi) with `tps` tiles per slot (slot = tile / tps gives the centre, the side and the pooled row); rows of conv[1], layer 3 and
    // layer 4 are indexed by the global row, pooled rows by tile (NOT merged over a slot's tiles)
    std::vector<float> r1((size_t)rows * 64), r3((size_t)rows * 128), rp((size_t)n_tiles * 512);
    int mixed = 0, dead_cols[2] = {0, 0};
    auto host = [&](int t_lo, int t_hi, int tps, bool stats) {
        for (int t = t_lo; t < t_hi; ++t) {
            const int slot = t / tps, side = slot & 1;
            std::vector<float> xc((size_t)32 * F), h[5], pre[5];
            for (int n = 0; n < 32; ++n)
                for (int c = 0; c < F; ++c) xc[(size_t)n * F + c] = x16[((size_t)t * 32 + n) * 16 + c] - cen[slot * 16 + c];
            layer_ref2(xc.data(), 32, F, w[side][0], b[side][0], 64, h[0], &pre[0]);
            for (int l = 1; l < 5; ++l) layer_ref2(h[l - 1].data(), 32, Ks[l], w[side][l], b[side][l], Ns[l], h[l], &pre[l]);
            memcpy(&r1[(size_t)t * 32 * 64], h[1].data(), 32 * 64 * 4);
            memcpy(&r3[(size_t)t * 32 * 128], h[3].data(), 32 * 128 * 4);
            for (int c = 0; c < 512; ++c) {
                float m = 0.f;
                bool pos = false;
                for (int n = 0; n < 32; ++n) { m = fmaxf(m, h[4][(size_t)n * 512 + c]); pos |= pre[4][(size_t)n * 512 + c] > 0.f; }
                rp[(size_t)t * 512 + c] = m;
                if (stats && !pos) ++dead_cols[t & 1];
            }
            if (stats)
                for (int l = 0; l < 3; ++l)
                    for (int n = 0; n < 32; ++n) {
                        bool neg[2] = {false, false}, pos[2] = {false, false};
                        for (int c = 0; c < 64; ++c) { const float v = pre[l][(size_t)n * 64 + c]; (v < 0.f ? neg : pos)[c >> 5] |= v != 0.f; }
                        mixed += (neg[0] && pos[1]) || (neg[1] && pos[0]);
                    }
        }
    };
    PArgs a;
    memset(&a, 0, sizeof(a));
    auto up = [&](const std::vector<float> &v) { float *dd; CK(hipMalloc(&dd, v.size() * 4)); CK(hipMemcpy(dd, v.data(), v.size() * 4, hipMemcpyHostToDevice)); return dd; };
    for (int side = 0; side < 2; ++side)
        for (int l = 0; l < 5; ++l) { a.w[side][l] = up(pk[side][l]); a.b[side][l] = up(b[side][l]); }
    a.x = up(x16); a.center = up(cen);
    float *conv1, *pool, *h3;
    CK(hipMalloc(&conv1, (size_t)rows * 64 * 4)); CK(hipMalloc(&h3, (size_t)rows * 128 * 4)); CK(hipMalloc(&pool, (size_t)n_tiles * 512 * 4));
    long long *cyc;
    CK(hipMalloc(&cyc, 256 * 2 * 8));
    a.conv1 = conv1; a.h3 = h3; a.pool = pool; a.cycles = cyc; a.iters = 1; a.tile_mod = 128;
    CK(hipFuncSetAttribute(reinterpret_cast<const void *>(pairs_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    std::vector<float> g1((size_t)rows * 64), g3((size_t)rows * 128), gp((size_t)n_tiles * 512);
    auto run = [&](int grid, int threads) {
        CK(hipMemset(conv1, 0xFF, (size_t)rows * 64 * 4)); CK(hipMemset(h3, 0xFF, (size_t)rows * 128 * 4)); CK(hipMemset(pool, 0, (size_t)n_tiles * 512 * 4));
        hipLaunchKernelGGL(pairs_kernel, dim3(grid), dim3(threads), P_LDS_FLOATS * 4, 0, a);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(g1.data(), conv1, g1.size() * 4, hipMemcpyDeviceToHost));
        CK(hipMemcpy(g3.data(), h3, g3.size() * 4, hipMemcpyDeviceToHost));
        CK(hipMemcpy(gp.data(), pool, gp.size() * 4, hipMemcpyDeviceToHost));
    };
    size_t bad = 0;
    if (roles) {
        // ---- `roles`: the teams of a register-tile CU by role (roles_kernel).  128 head tiles of a slot each beside the 128 branch tiles 2 .. 129 ----
        const int HT = 128, hrows = HT * 32;
        host(2, 130, 1, false);
        std::vector<float> hx((size_t)hrows * 64), hw0((size_t)64 * 256), hw1((size_t)256 * 128), hbv((size_t)HT * 256), hb1(128), fw(256), fb(2), pk0, pk1, lref;
        for (auto &v : hx) v = fmaxf(rnd(), 0.f) * 2.f;      // (conv[1] rows: behind a ReLU)
        for (auto &v : hw0) v = rnd() * 0.2f;
        for (auto &v : hw1) v = rnd() * 0.1f;
        for (auto &v : hbv) v = rnd() * 0.5f;
        for (auto *v : {&hb1, &fb}) for (auto &e : *v) e = rnd() * 0.1f;
        for (auto &v : fw) v = rnd() * 0.2f;
        pack(hw0, 64, 256, pk0); pack(hw1, 256, 128, pk1);
        head_ref(hx, hrows, 32, hw0, hbv, hw1, hb1, fw, fb, lref);
        LrgFusedProb &H = a.head;
        H.x = up(hx); H.L[0].w = up(pk0); H.L[0].bias = up(hbv); H.L[1].w = up(pk1); H.L[1].bias = up(hb1); H.fw = up(fw); H.fb = up(fb);
        float *lout; CK(hipMalloc(&lout, (size_t)hrows * 2 * 4)); H.fout = lout;
        CK(hipFuncSetAttribute(reinterpret_cast<const void *>(roles_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        std::vector<float> lg((size_t)hrows * 2);
        a.h3 = nullptr; a.tile0 = 2; a.tiles_per_team = 64; a.tiles_per_slot = 1; a.nparts = 1;
        struct Case { const char *name; int kind[2], timed; } cases[4] = {
            {"(a) a head tile alone", {2, 0}, 0}, {"(b) a head tile beside a head team", {2, 2}, 0},
            {"(c) a head tile beside a branch team", {1, 2}, 1}, {"(d) a branch tile, team 1 absent", {1, 0}, 0}};
        // values: every team runs its 64 tiles once, both teams to the end
        for (const Case &c : cases) {
            a.kind[0] = c.kind[0]; a.kind[1] = c.kind[1]; a.background = -1; a.iters = 1;
            CK(hipMemset(conv1, 0xFF, (size_t)rows * 64 * 4)); CK(hipMemset(pool, 0, (size_t)n_tiles * 512 * 4)); CK(hipMemset(lout, 0xFF, (size_t)hrows * 2 * 4));
            hipLaunchKernelGGL(roles_kernel, dim3(1), dim3(512), P_LDS_FLOATS * 4, 0, a);
            CK(hipDeviceSynchronize());
            CK(hipMemcpy(g1.data(), conv1, g1.size() * 4, hipMemcpyDeviceToHost));
            CK(hipMemcpy(gp.data(), pool, gp.size() * 4, hipMemcpyDeviceToHost));
            CK(hipMemcpy(lg.data(), lout, lg.size() * 4, hipMemcpyDeviceToHost));
            size_t bl = 0, nl = 0, b1 = 0, bp = 0, nb = 0;
            for (int t = 0; t < 2; ++t) {
                if (c.kind[t] == 2) { bl += differ(lg, lref, (size_t)t * 64 * 64, 64 * 64); nl += 64 * 64; }      // (team t's head tiles 64 t .. 64 t + 63: 32 rows x 2 logits each)
                if (c.kind[t] == 1) { b1 += differ(g1, r1, (size_t)(2 + 64 * t) * 32 * 64, (size_t)64 * 32 * 64); bp += differ(gp, rp, (size_t)(2 + 64 * t) * 512, 64 * 512); nb += 64; }
            }
            printf("roles %s, 64 tiles per team: logits %zu of %zu differ from the host chain; conv[1] %zu of %zu; pooled %zu of %zu\n", c.name, bl, nl, b1, nb * 32 * 64, bp, nb * 512);
            bad += bl + b1 + bp;
        }
        // ticks per tile of the timed team (64 tiles x 8), the other team -- where there is one -- running its tiles without pause until the timed one is through
        for (const Case &c : cases)
            for (int grid : {1, 200}) {
                a.kind[0] = c.kind[0]; a.kind[1] = c.kind[1]; a.background = (c.kind[0] && c.kind[1]) ? 1 - c.timed : -1; a.iters = 8;
                hipLaunchKernelGGL(roles_kernel, dim3(grid), dim3(512), P_LDS_FLOATS * 4, 0, a);
                CK(hipDeviceSynchronize());
                std::vector<long long> cy((size_t)grid * 2);
                CK(hipMemcpy(cy.data(), cyc, cy.size() * 8, hipMemcpyDeviceToHost));
                double sum = 0;
                for (int g = 0; g < grid; ++g) sum += (double)cy[g * 2 + c.timed] / (a.iters * a.tiles_per_team);
                printf("ROLES %s, grid %3d: %8.0f counter ticks per tile\n", c.name, grid, sum / grid);
            }
        return bad ? 1 : 0;
    }
    // ---- single tiles: tile 0 on side 0, tile 1 on side 1 (a slot each), one workgroup (one team) per tile ----
    host(0, 2, 1, true);
    printf("single tile inputs: %d of %d (point, layer) of layers 0 - 2 have a negative pre-activation in one block and a positive one in the other; "
           "%d + %d pooled columns are non-positive for every point\n", mixed, 2 * 3 * 32, dead_cols[0], dead_cols[1]);
    for (int nparts = 1; nparts <= 2; ++nparts) {
        a.tile0 = 0; a.tiles_per_team = 1; a.tiles_per_slot = 1; a.nparts = nparts;
        run(2, 256);
        const size_t b1 = differ(g1, r1, 0, 2 * 32 * 64), b3 = differ(g3, r3, 0, 2 * 32 * 128), bp = differ(gp, rp, 0, 2 * 512);
        printf("single tile, %d part(s): conv[1] %zu of %d differ; layer 3 %zu of %d; pooled %zu of %d\n", nparts, b1, 2 * 32 * 64, b3, 2 * 32 * 128, bp, 2 * 512);
        bad += b1 + b3 + bp;
    }
    // ---- two tiles of one slot: one pooled row, the column-wise maximum of the two tiles' host rows ----
    {
        host(0, 2, 2, false);
        std::vector<float> want(512);
        size_t from0 = 0, from1 = 0;
        for (int c = 0; c < 512; ++c) { want[c] = fmaxf(rp[c], rp[512 + c]); from0 += rp[c] > rp[512 + c]; from1 += rp[512 + c] > rp[c]; }
        a.tile0 = 0; a.tiles_per_team = 1; a.tiles_per_slot = 2; a.nparts = 1;
        run(2, 256);
        const size_t bp = differ(gp, want, 0, 512), b1 = differ(g1, r1, 0, 2 * 32 * 64);
        printf("two tiles, one pooled row: pooled %zu of 512 differ from the column-wise maximum of the two host rows (%zu columns from tile 0, %zu from tile 1); conv[1] %zu differ\n",
               bp, from0, from1, b1);
        bad += bp + b1;
    }
    // ---- both teams of one workgroup, 64 different tiles each, back to back ----
    {
        host(2, 130, 1, false);
        a.tile0 = 2; a.tiles_per_team = 64; a.tiles_per_slot = 1; a.nparts = 1;
        run(1, 512);
        const size_t b1 = differ(g1, r1, (size_t)2 * 32 * 64, (size_t)128 * 32 * 64), b3 = differ(g3, r3, (size_t)2 * 32 * 128, (size_t)128 * 32 * 128), bp = differ(gp, rp, 2 * 512, 128 * 512);
        printf("both teams, 64 tiles each: conv[1] %zu of %d differ; layer 3 %zu of %d; pooled %zu of %d\n", b1, 128 * 32 * 64, b3, 128 * 32 * 128, bp, 128 * 512);
        bad += b1 + b3 + bp;
    }
    // ---- timing: a team of a 512-thread workgroup alone, beside a second branch team, beside a head team (counter ticks per tile, 64 tiles x 8) ----
    {
        std::vector<float> hx((size_t)64 * 32 * 64), hw0((size_t)64 * 256), hw1((size_t)256 * 128), hb0(256), hb1(128), fw(256), fb(2), pk0, pk1;
        for (auto *v : {&hx, &hw0, &hw1, &hb0, &hb1, &fw, &fb}) for (auto &e : *v) e = rnd() * 0.2f;
        pack(hw0, 64, 256, pk0); pack(hw1, 256, 128, pk1);
        LrgFusedProb &H = a.head;
        H.x = up(hx); H.L[0].w = up(pk0); H.L[0].bias = up(hb0); H.L[1].w = up(pk1); H.L[1].bias = up(hb1); H.fw = up(fw); H.fb = up(fb);
        float *lout; CK(hipMalloc(&lout, (size_t)64 * 32 * 2 * 4)); H.fout = lout;
        a.h3 = nullptr; a.tile0 = 2; a.tiles_per_team = 64; a.tiles_per_slot = 1; a.nparts = 1; a.iters = 8;
        const char *names[3] = {"alone", "beside a second branch team", "beside a head team"};
        for (int mode = 0; mode < 3; ++mode)
            for (int grid : {1, 200}) {
                a.head_beside = mode == 2;
                hipLaunchKernelGGL(pairs_kernel, dim3(grid), dim3(mode ? 512 : 256), P_LDS_FLOATS * 4, 0, a);
                CK(hipDeviceSynchronize());
                std::vector<long long> c((size_t)grid * 2);
                CK(hipMemcpy(c.data(), cyc, c.size() * 8, hipMemcpyDeviceToHost));
                double sum = 0;
                for (int g = 0; g < grid; ++g) sum += (double)c[g * 2] / (a.iters * a.tiles_per_team);
                printf("REGISTER TILE as a worker's team, %s, grid %3d: %8.0f counter ticks per tile\n", names[mode], grid, sum / grid);
            }
    }
    return bad ? 1 : 0;
}

// ---- mode `units`: sixteen pooled-product units of one form and a driver workgroup in the front workgroups' place ----
// Thread i of the driver owns slot i: it writes the slot's ring entry as the last branch tile would (a ticket from LRG_AQ_GTAIL, the tagged entry), waits for the
// sixteen arrivals on the slot's sync[1] and writes the next, `rounds` times; then the driver counts itself among the fronts that are done and the units leave.
// One active slot: a task at a time, the ticks from the entry's store to the sixteenth arrival seen are the stage's latency.  96 active slots: the ring is kept
// full and the tasks per second are the units' capacity.  Every wait is bounded by abort_ticks (one second), as in a launch.
struct UArgs { int form, n_active, rounds; unsigned long long *out; };      // out: [0] ticks from the first entry to the last arrival, [1] ticks entry -> arrival, summed
__global__ __launch_bounds__(LRG_FRONT_THREADS) void units_kernel(LrgAsyncKArgs K, UArgs u) {
    const long long t_launch = wall_clock64();
#if defined(__HIP_DEVICE_COMPILE__)
    lrg_kargs_ptr kp = (lrg_kargs_ptr)__builtin_amdgcn_kernarg_segment_ptr();
#else
    lrg_kargs_ptr kp = nullptr;
#endif
    if (blockIdx.x >= 1) {
        const int unit = (int)blockIdx.x - 1;
        if (u.form == 3) lrg_async_gemv_unit3(kp, unit, t_launch);
        else if (u.form == 2) lrg_async_gemv_unit2(kp, unit, t_launch);
        else lrg_async_gemv_unit(kp, unit, t_launch);
        return;
    }
    const LrgAsyncArgs &A = K.A;
    const int slot = threadIdx.x;
    int32_t *sy = A.sync + (long)slot * LRG_ASYNC_SYNC_WORDS;
    int issued = 0, done = 0;
    long long t_issue = 0, lat = 0;
    if (slot < u.n_active)
        for (unsigned spin = 1; done < u.rounds; ++spin) {
            if (issued == done) {
                const int nt_in = 1 + (slot & 15), nt_nb = 16 - (slot & 15);
                const int i = __hip_atomic_fetch_add(&A.queue[LRG_AQ_GTAIL], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                t_issue = wall_clock64();
                lrg_st_coh(&A.queue[LRG_AQ_RING + 2 * (A.qmask + 1) + (i & A.gmask)], (lrg_gemv_ring_tag(i, A.gmask) << 20) | ((nt_in - 1) << 16) | ((nt_nb - 1) << 12) | slot);
                ++issued;
            } else if (lrg_ld_coh(&sy[1]) >= A.gemv_units * issued) {
                lat += wall_clock64() - t_issue;
                ++done;
            } else {
                if ((spin & 255u) == 0 && (lrg_ld_coh(&A.queue[LRG_AQ_ABORT]) || wall_clock64() - t_launch > A.abort_ticks)) { lrg_st_coh(&A.queue[LRG_AQ_ABORT], 9); break; }
                __builtin_amdgcn_s_sleep(1);
            }
        }
    if (slot < u.n_active) atomicAdd(&u.out[1], (unsigned long long)lat);
    __syncthreads();
    if (threadIdx.x == 0) {
        u.out[0] = (unsigned long long)(wall_clock64() - t_launch);
        __hip_atomic_fetch_add(&A.queue[LRG_AQ_FRONTS_DONE], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

static int units_main() {
    const int P = 1024, C = 256, S = 96, TILES = 16, ROUNDS = 8;
    srand(2024);
    auto rnd = []() { return (float)rand() / RAND_MAX * 2.f - 1.f; };
    std::vector<float> w[2], bias[2], pooled((size_t)S * P), prow((size_t)S * 2 * TILES * (P / 2)), pooled_max((size_t)S * P, 0.f);
    for (int z = 0; z < 2; ++z) {
        w[z].resize((size_t)P * C); bias[z].resize(C);
        for (auto &v : w[z]) v = rnd() * 0.05f;
        for (auto &v : bias[z]) v = rnd() * 0.1f;
    }
    for (auto &v : pooled) { v = rnd() * 3.f; if (v < 0.f) v = 0.f; }      // (pooled features are maxima of ReLU outputs: about half of them zero here)
    // per-tile pool rows: slot s has 1 + s % 16 inlier tiles and 16 - s % 16 neighbour tiles (1 and 16 of either among them); the rows of tiles it does not have hold
    // a huge value that no maximum may pick up
    for (int s = 0; s < S; ++s)
        for (int side = 0; side < 2; ++side) {
            const int nt = side ? 16 - (s & 15) : 1 + (s & 15);
            for (int t = 0; t < TILES; ++t)
                for (int c = 0; c < P / 2; ++c) {
                    float v = rnd() * 3.f;
                    if (v < 0.f) v = 0.f;
                    if (t >= nt) v = 3e38f;
                    prow[(((size_t)s * 2 + side) * TILES + t) * (P / 2) + c] = v;
                    if (t < nt) pooled_max[(size_t)s * P + side * (P / 2) + c] = fmaxf(pooled_max[(size_t)s * P + side * (P / 2) + c], v);
                }
        }
    // the host chain: eight K ranges of 128, in a range one chain of fmaf over k = 8g + 0, 4, 1, 5, 2, 6, 3, 7 for g ascending, the eight partial sums in order, the bias
    auto host = [&](const std::vector<float> &rows, std::vector<float> &out) {
        out.assign((size_t)2 * S * C, 0.f);
        static const int perm[8] = {0, 4, 1, 5, 2, 6, 3, 7};
        for (int z = 0; z < 2; ++z)
            for (int s = 0; s < S; ++s)
                for (int c = 0; c < C; ++c) {
                    float part[8];
                    for (int r = 0; r < 8; ++r) {
                        float acc = 0.f;
                        for (int g = 0; g < 16; ++g)
                            for (int j = 0; j < 8; ++j) { const int k = r * 128 + 8 * g + perm[j]; acc = fmaf(rows[(size_t)s * P + k], w[z][(size_t)k * C + c], acc); }
                        part[r] = acc;
                    }
                    float sum = part[0];
                    for (int r = 1; r < 8; ++r) sum += part[r];
                    out[((size_t)z * S + s) * C + c] = sum + bias[z][c];
                }
    };
    std::vector<float> ref_row, ref_max;
    host(pooled, ref_row); host(pooled_max, ref_max);
    auto up = [&](const std::vector<float> &v) { float *dd; CK(hipMalloc(&dd, v.size() * 4)); CK(hipMemcpy(dd, v.data(), v.size() * 4, hipMemcpyHostToDevice)); return dd; };
    static LrgAsyncKArgs K;
    memset(static_cast<void *>(&K), 0, sizeof(K));
    LrgAsyncArgs &A = K.A;
    float *hb, *d_prow = up(prow);
    CK(hipMalloc(&hb, (size_t)2 * S * C * 4));
    A.gemv.pooled = up(pooled);
    for (int z = 0; z < 2; ++z) { A.gemv.w[z] = up(w[z]); A.gemv.bias[z] = up(bias[z]); A.gemv.hb[z] = hb + (size_t)z * S * C; }
    A.gemv.ldw = C; A.gemv.B = S; A.gemv.P = P; A.gemv.C = C;
    A.qmask = 63; A.gmask = 255;                 // (a units' ring of 256 entries: 96 slots x 8 rounds go round it three times)
    const size_t queue_words = LRG_AQ_RING + 2 * (A.qmask + 1) + (A.gmask + 1) + 64;
    CK(hipMalloc(&A.queue, queue_words * 4)); CK(hipMalloc(&A.sync, (size_t)S * LRG_ASYNC_SYNC_WORDS * 4));
    A.n_slots = S; A.n_front = 1; A.gemv_units = 2 * C / LRG_GEMV_UNIT_COLS; A.pool_rows_stride = 2 * TILES * (P / 2);
    A.abort_ticks = 100000000LL;                 // one second
    unsigned long long *out;
    CK(hipMalloc(&out, 16));
    const size_t lds = (size_t)std::max((int)LRG_GEMV_UNIT_FLOATS(P), (int)LRG_GEMV_UNIT2_FLOATS(P)) * 4 + 16;      // (what lrg_async_plan gives the units)
    static_assert(LRG_GEMV_UNIT3_FLOATS <= LRG_GEMV_UNIT_FLOATS(1024), "the register form's FIFO within the units' LDS");
    CK(hipFuncSetAttribute(reinterpret_cast<const void *>(units_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    std::vector<float> got((size_t)2 * S * C);
    std::vector<int32_t> sy((size_t)S * LRG_ASYNC_SYNC_WORDS), q(queue_words);
    unsigned long long res[2];
    // one launch: returns the abort word (0: every wait ended by itself)
    auto launch = [&](int form, bool pool_rows, int n_active, int rounds) {
        CK(hipMemset(A.queue, 0, queue_words * 4)); CK(hipMemset(A.sync, 0, sy.size() * 4)); CK(hipMemset(out, 0, 16)); CK(hipMemset(hb, 0xFF, got.size() * 4));
        A.pool_rows = pool_rows ? d_prow : nullptr;
        UArgs u; u.form = form; u.n_active = n_active; u.rounds = rounds; u.out = out;
        hipLaunchKernelGGL(units_kernel, dim3(1 + A.gemv_units), dim3(LRG_FRONT_THREADS), lds, 0, K, u);
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(got.data(), hb, got.size() * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(sy.data(), A.sync, sy.size() * 4, hipMemcpyDeviceToHost));
        CK(hipMemcpy(q.data(), A.queue, q.size() * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(res, out, 16, hipMemcpyDeviceToHost));
        return q[LRG_AQ_ABORT];
    };
    static const char *const names[4] = {"", "four teams", "half-teams", "registers"};
    size_t bad_all = 0;
    for (int form = 1; form <= 3; ++form) {
        for (int pr = 0; pr < 2; ++pr) {
            if (pr && form == 2) continue;       // (the half-teams do not take per-tile pool rows: the kernel gives those launches the four-team form)
            const int aborted = launch(form, pr, S, ROUNDS);
            const std::vector<float> &ref = pr ? ref_max : ref_row;
            const size_t bad = differ(got, ref, 0, got.size());
            int complete = 0;
            for (int s = 0; s < S; ++s) complete += sy[(size_t)s * LRG_ASYNC_SYNC_WORDS + 1] == A.gemv_units * ROUNDS;
            printf("units form %d (%s), %s: sums %zu of %zu differ from the host chain; slots with all arrivals %d of %d; abort word %d\n", form, names[form],
                   pr ? "per-tile pool rows" : "pooled rows", bad, got.size(), complete, S, aborted);
            for (size_t i = 0, shown = 0; i < got.size() && shown < 6; ++i)
                if (memcmp(&got[i], &ref[i], 4)) { printf("  head %zu slot %zu column %zu: gpu %.9g ref %.9g\n", i / ((size_t)S * C), i / C % S, i % C, got[i], ref[i]); ++shown; }
            bad_all += bad + (size_t)(S - complete) + (aborted ? 1 : 0);
            if (aborted) return 1;               // (a wait ran into its bound: nothing more is started)
        }
        int aborted = launch(form, false, 1, 2000);
        printf("UNITS form %d (%s) latency: %8.0f ticks of 10 ns from the entry written to the sixteenth arrival seen, one task at a time (abort word %d)\n", form, names[form],
               (double)res[1] / 2000.0, aborted);
        if (aborted) return 1;
        aborted = launch(form, false, S, 200);
        printf("UNITS form %d (%s) capacity: %8.0f k tasks/s per unit with %d slots' entries kept in the ring (%d tasks in %llu ticks; abort word %d)\n", form, names[form],
               (double)S * 200 / ((double)res[0] * 1e-8) * 1e-3, S, S * 200, res[0], aborted);
        if (aborted) return 1;
    }
    return bad_all ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "pairs")) return pairs_main(false);
    if (argc > 1 && !strcmp(argv[1], "units")) return units_main();
    if (argc > 1 && !strcmp(argv[1], "roles")) return pairs_main(true);
    const int n_slots = 6, rows_per_slot = 96, rows = n_slots * rows_per_slot, n_tiles = rows / 32, F = 13;
    const int Ks[5] = {F, 64, 64, 64, 128}, Ns[5] = {64, 64, 64, 128, 512};
    srand(12345);
    auto rnd = []() { return (float)rand() / RAND_MAX * 2.f - 1.f; };
    std::vector<float> w[5], b[5], pk[5];
    for (int l = 0; l < 5; ++l) {
        w[l].resize((size_t)Ks[l] * Ns[l]); b[l].resize(Ns[l]);
        const float sc = 1.5f / sqrtf((float)Ks[l]);
        for (auto &v : w[l]) v = rnd() * sc;
        for (auto &v : b[l]) v = rnd() * 0.1f;
        pack(w[l], Ks[l], Ns[l], pk[l]);
    }
    std::vector<float> x16((size_t)rows * 16, 0.f), cen((size_t)n_slots * 16, 0.f), xc((size_t)rows * F);
    for (int s = 0; s < n_slots; ++s)
        for (int c = 0; c < F; ++c) cen[s * 16 + c] = (c < 2 || c >= 6) ? rnd() : 0.f;
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < F; ++c) {
            x16[(size_t)r * 16 + c] = rnd() * 2.f;
            xc[(size_t)r * F + c] = x16[(size_t)r * 16 + c] - cen[(r / rows_per_slot) * 16 + c];
        }
    // host reference
    std::vector<float> h[5];
    layer_ref(xc, rows, F, w[0], b[0], 64, h[0]);
    for (int l = 1; l < 5; ++l) layer_ref(h[l - 1], rows, Ks[l], w[l], b[l], Ns[l], h[l]);
    std::vector<float> pool_ref((size_t)n_slots * 512, 0.f);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < 512; ++c) pool_ref[(size_t)(r / rows_per_slot) * 512 + c] = fmaxf(pool_ref[(size_t)(r / rows_per_slot) * 512 + c], h[4][(size_t)r * 512 + c]);

    Args a;
    float *d;
    for (int l = 0; l < 5; ++l) {
        CK(hipMalloc(&d, pk[l].size() * 4)); CK(hipMemcpy(d, pk[l].data(), pk[l].size() * 4, hipMemcpyHostToDevice)); a.w[l] = d;
        CK(hipMalloc(&d, b[l].size() * 4)); CK(hipMemcpy(d, b[l].data(), b[l].size() * 4, hipMemcpyHostToDevice)); a.b[l] = d;
    }
    CK(hipMalloc(&d, x16.size() * 4)); CK(hipMemcpy(d, x16.data(), x16.size() * 4, hipMemcpyHostToDevice)); a.x = d;
    CK(hipMalloc(&d, cen.size() * 4)); CK(hipMemcpy(d, cen.data(), cen.size() * 4, hipMemcpyHostToDevice)); a.center = d;
    float *conv1, *pool, *h3;
    CK(hipMalloc(&conv1, (size_t)rows * 64 * 4)); CK(hipMemset(conv1, 0xFF, (size_t)rows * 64 * 4));
    CK(hipMalloc(&h3, (size_t)rows * 128 * 4)); CK(hipMemset(h3, 0xFF, (size_t)rows * 128 * 4));
    CK(hipMalloc(&pool, (size_t)n_slots * 512 * 4)); CK(hipMemset(pool, 0, (size_t)n_slots * 512 * 4));
    long long *cyc;
    CK(hipMalloc(&cyc, 256 * 16 * 8));
    a.conv1 = conv1; a.h3 = h3; a.pool = pool; a.cycles = cyc; a.n_tiles = n_tiles; a.rows_per_slot = rows_per_slot;
    CK(hipFuncSetAttribute(reinterpret_cast<const void *>(probe_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    const size_t lds = LRG_WB_FLOATS * 4;

    // ---- correctness: every tile's PREFIX task, then every (tile, quarter) POOL task, at least once ----
    a.iters = 1; a.waves = 4;
    const int wgs = 2 * ((n_tiles + 3) / 4) * 2;      // (each tile several times: the stores and the maxima are idempotent)
    a.stage = 0;
    hipLaunchKernelGGL(probe_kernel, dim3(wgs), dim3(512), lds, 0, a);
    CK(hipDeviceSynchronize());
    a.stage = 1;
    hipLaunchKernelGGL(probe_kernel, dim3(2 * wgs), dim3(512), lds, 0, a);
    CK(hipDeviceSynchronize());
    std::vector<float> g1((size_t)rows * 64), g3((size_t)rows * 128), gp((size_t)n_slots * 512);
    CK(hipMemcpy(g1.data(), conv1, g1.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(g3.data(), h3, g3.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(gp.data(), pool, gp.size() * 4, hipMemcpyDeviceToHost));
    size_t bad1 = 0, bad3 = 0, badp = 0;
    for (size_t i = 0; i < g1.size(); ++i) bad1 += memcmp(&g1[i], &h[1][i], 4) != 0;
    for (size_t i = 0; i < g3.size(); ++i) bad3 += memcmp(&g3[i], &h[3][i], 4) != 0;
    for (size_t i = 0; i < gp.size(); ++i) badp += memcmp(&gp[i], &pool_ref[i], 4) != 0;
    printf("conv[1]: %zu of %zu values differ from the host chain; layer 3: %zu of %zu; pooled: %zu of %zu\n", bad1, g1.size(), bad3, g3.size(), badp, gp.size());
    if (bad1 || bad3 || badp) {
        for (size_t i = 0, shown = 0; i < g1.size() && shown < 8; ++i)
            if (memcmp(&g1[i], &h[1][i], 4)) { printf("  conv1[%zu,%zu] gpu %.9g ref %.9g\n", i / 64, i % 64, g1[i], h[1][i]); ++shown; }
        for (size_t i = 0, shown = 0; i < gp.size() && shown < 8; ++i)
            if (memcmp(&gp[i], &pool_ref[i], 4)) { printf("  pool[%zu,%zu] gpu %.9g ref %.9g\n", i / 512, i % 512, gp[i], pool_ref[i]); ++shown; }
    }
    badp += bad3;
    // ---- the register tile (a team of four wavefronts per tile) ----
    CK(hipMemset(conv1, 0xFF, (size_t)rows * 64 * 4)); CK(hipMemset(pool, 0, (size_t)n_slots * 512 * 4));
    a.stage = 2; a.iters = 1;
    hipLaunchKernelGGL(probe_kernel, dim3(n_tiles), dim3(256), (LRG_RT_WEIGHT_FLOATS + LRG_RT_XCH_FLOATS) * 4, 0, a);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(g1.data(), conv1, g1.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(gp.data(), pool, gp.size() * 4, hipMemcpyDeviceToHost));
    size_t rb1 = 0, rbp = 0;
    for (size_t i = 0; i < g1.size(); ++i) rb1 += memcmp(&g1[i], &h[1][i], 4) != 0;
    for (size_t i = 0; i < gp.size(); ++i) rbp += memcmp(&gp[i], &pool_ref[i], 4) != 0;
    printf("register tile (team of four): conv[1] %zu of %zu differ; pooled %zu of %zu\n", rb1, g1.size(), rbp, gp.size());
    badp += rb1 + rbp;
    for (int grid : {1, 200}) {
        a.iters = 50;
        hipLaunchKernelGGL(probe_kernel, dim3(grid), dim3(256), (LRG_RT_WEIGHT_FLOATS + LRG_RT_XCH_FLOATS) * 4, 0, a);
        CK(hipDeviceSynchronize());
        std::vector<long long> c((size_t)grid * 16);
        CK(hipMemcpy(c.data(), cyc, c.size() * 8, hipMemcpyDeviceToHost));
        double sum = 0;
        for (int g = 0; g < grid; ++g) sum += (double)c[g * 16] / a.iters;
        printf("REGISTER TILE, grid %3d, one team per CU: %8.0f counter ticks per tile (the team tile of lrg_fused_tile.inl: ~52 000)\n", grid, sum / grid);
    }

    // ---- timing (counter ticks of the shader clock; a PREFIX task is 272 x 64 = 17 408 cycles of MFMA issue, a POOL task 256 x 64 = 16 384) ----
    int dev = 0;
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, dev));
    const double ghz = prop.clockRate * 1e-6;
    for (int stage = 0; stage < 2; ++stage)
        for (int grid : {2, 200}) {
            for (int waves : {1, 4, 8}) {
                a.iters = 50; a.waves = waves; a.stage = stage;
                hipLaunchKernelGGL(probe_kernel, dim3(grid), dim3(512), lds, 0, a);
                CK(hipDeviceSynchronize());
                std::vector<long long> c((size_t)grid * 16);
                CK(hipMemcpy(c.data(), cyc, c.size() * 8, hipMemcpyDeviceToHost));
                double sum = 0, mx = 0;
                for (int g = 0; g < grid; ++g)
                    for (int wv = 0; wv < waves; ++wv) { const double v = (double)c[g * 16 + wv] / a.iters; sum += v; mx = v > mx ? v : mx; }
                printf("%s, grid %3d, %2d waves per CU: %8.0f counter ticks per task (max %8.0f)\n", stage ? "POOL  " : "PREFIX", grid, waves, sum / (grid * waves), mx);
            }
        }
    // ---- the register head tile: conv[1] rows (the branch reference's) + a per-slot pooled product -> 256 -> 128 -> 2 ----
    {
        std::vector<float> hw0((size_t)64 * 256), hw1((size_t)256 * 128), hbias1(128), fw(256), fb(2), hbv((size_t)n_slots * 256), pk0, pk1;
        for (auto &v : hw0) v = rnd() * 0.2f;
        for (auto &v : hw1) v = rnd() * 0.1f;
        for (auto &v : hbias1) v = rnd() * 0.1f;
        for (auto &v : fw) v = rnd() * 0.2f;
        for (auto &v : fb) v = rnd() * 0.1f;
        for (auto &v : hbv) v = rnd() * 0.5f;
        pack(hw0, 64, 256, pk0); pack(hw1, 256, 128, pk1);
        // host: head_ref above
        std::vector<float> lref;
        const std::vector<float> &cin = h[1];
        head_ref(cin, rows, rows_per_slot, hw0, hbv, hw1, hbias1, fw, fb, lref);
        auto up = [&](const std::vector<float> &v) { float *dd; CK(hipMalloc(&dd, v.size() * 4)); CK(hipMemcpy(dd, v.data(), v.size() * 4, hipMemcpyHostToDevice)); return dd; };
        LrgFusedProb &H = a.head;
        memset(&H, 0, sizeof(H));
        H.x = up(cin); H.L[0].w = up(pk0); H.L[0].bias = up(hbv); H.L[1].w = up(pk1); H.L[1].bias = up(hbias1); H.fw = up(fw); H.fb = up(fb);
        float *lout; CK(hipMalloc(&lout, (size_t)rows * 2 * 4)); CK(hipMemset(lout, 0xFF, (size_t)rows * 2 * 4)); H.fout = lout;
        a.stage = 3; a.iters = 1;
        hipLaunchKernelGGL(probe_kernel, dim3(n_tiles), dim3(256), LRG_RH_FLOATS * 4, 0, a);
        CK(hipDeviceSynchronize());
        std::vector<float> lg((size_t)rows * 2);
        CK(hipMemcpy(lg.data(), lout, lg.size() * 4, hipMemcpyDeviceToHost));
        size_t bl = 0;
        for (size_t i = 0; i < lg.size(); ++i) bl += memcmp(&lg[i], &lref[i], 4) != 0;
        printf("register head tile: logits %zu of %zu differ from the host chain\n", bl, lg.size());
        for (size_t i = 0, shown = 0; i < lg.size() && shown < 6; ++i) if (memcmp(&lg[i], &lref[i], 4)) { printf("  logit[%zu,%zu] gpu %.9g ref %.9g\n", i / 2, i % 2, lg[i], lref[i]); ++shown; }
        badp += bl;
        for (int grid : {1, 200}) {
            a.iters = 50;
            hipLaunchKernelGGL(probe_kernel, dim3(grid), dim3(256), LRG_RH_FLOATS * 4, 0, a);
            CK(hipDeviceSynchronize());
            std::vector<long long> c((size_t)grid * 16);
            CK(hipMemcpy(c.data(), cyc, c.size() * 8, hipMemcpyDeviceToHost));
            double sum = 0;
            for (int g = 0; g < grid; ++g) sum += (double)c[g * 16] / a.iters;
            printf("REGISTER HEAD TILE, grid %3d, one team per CU: %8.0f counter ticks per tile\n", grid, sum / grid);
        }
    }
    (void)ghz;
    (void)argc; (void)argv;
    return (bad1 || badp) ? 1 : 0;
}
