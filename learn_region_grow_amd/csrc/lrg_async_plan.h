// Internal interface of the free-running launch (lrg_grow_async): the arguments of its kernels (lrg_front.inl, lrg_async.inl), the layout of its queue and the
// launch plan that lrg_async_plan.inl decides.  Structs and host declarations only: a translation unit without a kernel can include it
// (tools/async_plan_table.hip prints the plans of a fixed sweep, tests/test_async_plan.py compares them with tests/golden/async_plan_table.txt).
#pragma once
#include "lrg_fused.h"

// ---- the front kernels' arguments (lrg_front.inl) ----
struct LrgFrontArgs {
    float *center;
    int32_t *sample_in, *sample_nb;
    float *x_in, *x_nb;
    int32_t *row_slot_in, *row_slot_nb;
    float4 *upd_in, *upd_nb; // [n_slots, n_inlier] / [n_slots, n_neighbor]: (x, y, z as stored in the packed row, ground-truth flag) of the
                             // slot's distinct rows -- what the NEXT mask update needs of them, in storage of the slot's own.  The packed
                             // arrays are re-allocated from row 0 by every launch: a workgroup that starts late (the chip busy with
                             // another lane's kernels) would find its rows of the last iteration overwritten by the slots that are
                             // already gathering.
    const float *rmv_logits, *add_logits;
    int32_t *slot_rows;      // [n_slots,4]: rows_in, rows_nb, first packed inlier row, first packed neighbour row
    int32_t *counters;       // [0] packed inlier rows, [1] packed neighbour rows allocated so far in this iteration
    float *pooled;           // [n_slots, pooled_stride] pooled features of the network workspace (zeroed here per slot)
    int pooled_stride;
    int64_t *stats;
    int64_t *phase_ticks;    // nullable: [n_slots,2] wall-clock ticks per slot: (0) update / stop / commit, (1) query / median / gather
    int own_medians;         // greedy front kernel: 1 = every slot's workgroup computes its nine medians itself (no launch of their own)
    unsigned long long *phase_dbg;   // nullable (free-running kernel): [8] accumulated wall-clock ticks of the front's phases; [9 .. 11] inside the mask update: entry -> the
                                     // slot's words in use, -> logits in registers, -> `take` known
    int row_stride;          // free-running kernel: slot s owns the rows [s * row_stride, (s + 1) * row_stride) of the row arrays
    int rows16;              // free-running kernel: 1 = the gathered rows are written at a 64-byte stride (16 floats, zero-padded) in 16-byte pieces
    int fill_in_launch;      // free-running kernel: finished rooms are filled in (:308-316) by tile teams of the same launch -- flagged in the done ring (bit 31 of the slot word)
    // free-running kernel, shared tail tiles (lrg_async.inl): a slot's rows beyond its last FULL 32-row tile go to rows that the slots share, reserved from a cursor
    // per side -- several slots' tails fill one tile instead of each padding a tile of its own.  nullable (then every slot pads its own tail, as before).
    int32_t *tail_cur;       // [0] / [16]: rows reserved so far on the inlier / neighbour side (one 64-byte line each)
    int32_t *tail_base;      // [n_slots][2]: where the slot's tail rows of its evaluation in flight start in the shared rows (-1: in its own place)
    int tail_rows;           // shared rows per side (a multiple of 32)
    int tail_row0;           // first shared row in the row arrays (= n_slots * row_stride)
    unsigned long long *spec_stats;      // nullable: [0] regions voided by an earlier commit, [1] evaluations those regions had taken, [2] of them: mask updates done, i.e. steps the
                                         // device's step counter holds that no committed region keeps (LrgAsyncBuffers.work + 4)
    int spec_k;              // free-running kernel: K > 1 = speculation -- the slots g K .. g K + K - 1 grow the regions of the next K unvisited seeds of ONE room
                             // side by side (LrgAsyncBuffers.speculate; see "speculation" below); 0 / 1 = one slot, one room
};

// ---- the queue of a free-running launch (lrg_async.inl) ----
#define LRG_AQ_TAIL 0            // control words of the queue (ints), one 64-byte line each; ring 1 (pooled blocks and head tiles when
#define LRG_AQ_HEAD 16           // the workgroups run more than one team): + LRG_AQ_SECOND
#define LRG_AQ_FRONTS_DONE 32
#define LRG_AQ_ABORT 48
#define LRG_AQ_SECOND 64
#define LRG_AQ_GTAIL 96          // entries written to the pooled-product units' ring so far
#define LRG_AQ_ARRIVED 112       // workgroups of this launch that have started (the start rendezvous of the front workgroups)
#ifndef LRG_ASYNC_START_TICKS
#define LRG_ASYNC_START_TICKS 2000000LL      // 20 ms (wall_clock64: 100 MHz): by then every workgroup of the launch has started, or never will while the others wait
#endif
#define LRG_AQ_FTAIL 128         // the fill-in ring (tasks of the in-launch 1-NN fill-in, test_region_grow.py:308-316): entries reserved / taken
#define LRG_AQ_FHEAD 144
#define LRG_AQ_RING 192          // ring 0, then ring 1 (qmask + 1 entries each), then the units' ring (gmask + 1 entries), then the fill-in ring (fmask + 1)
#define LRG_ASYNC_FILL_RING 8192 // entries of the fill-in ring: one per 256 candidate points of a finished room (a 131 072-point scene: 512)
// behind the fill-in ring: the wave rings' control words (ring t = side * 4 + quarter: [32 t] entries reserved, [32 t + 16] tickets taken) and the eight rings
#define LRG_AQ_WAVE(A) (LRG_AQ_RING + 2 * ((A).qmask + 1) + ((A).gmask + 1) + LRG_ASYNC_FILL_RING)
#define LRG_AQ_WAVE_RING(A, t) (LRG_AQ_WAVE(A) + 256 + (t) * ((A).wmask + 1))

struct LrgAsyncArgs {
    LrgFusedProb prob[4];        // 0 inlier branch, 1 neighbour branch, 2 add head (neighbour rows), 3 remove head (inlier rows)
    LrgGemvArgs gemv;
    LrgFrontArgs front;
    int32_t *queue;              // control words + ring
    int32_t *sync;               // [n_slots, LRG_ASYNC_SYNC_WORDS]
    int32_t *big;
    int32_t *room_queue;         // nullable: [0] rooms handed out so far, [1] rooms queued, [2 + k] = room index | reset << 30
    int qmask;                   // ring entries - 1 (power of two)
    int gmask;                   // entries of the pooled-product units' ring - 1 (power of two, at least 2 n_slots)
    int gemv_batch;              // > 1 (without the units): pooled products in batches of up to so many slots (LRG_GEMV_BATCH) -- the slots whose branch tiles are all in
                                 // queue up in the (otherwise unused) units' ring; a batch's blocks stream the kernels' 128 columns ONCE for all its slots
    long long gemv_batch_ticks;  // a batch that is not full that long after its leader task was taken is closed with the slots it has
    int gemv_units;              // workgroups n_front .. n_front + gemv_units - 1 hold 32 columns each of the heads' pooled kernels in LDS (0: the
                                 // pooled product is a task of the tile teams, 128 columns each)
    int n_slots, n_front, teams;
    int head_ring;               // the ring pooled blocks and head tiles are published to: 1, or 0 = one ring for all tasks and all teams
    int ring0_halves;            // more than one team per workgroup: team t of worker workgroup w runs branch tiles (ring 0) if 2 t + (w & 1) < ring0_halves,
                                 // else pooled blocks and head tiles (ring 1) -- 2: the first team everywhere, 3: one and a half teams on average, ...
    // in-launch fill-in (nullable: fill_list == nullptr -> the host fills finished rooms in between launches)
    int32_t *fill_list;          // [points of all rooms] per room (at the room's offset in the arenas): indices of its unlabeled points
    unsigned long long *fill_best;   // [points of all rooms] best (distance bits << 32 | index) per point
    int32_t *fill_sync;          // [n_rooms, 4]: unlabeled points, candidate chunks done, chunks in all, filled
    const int32_t *fill_label_base;  // the label arena (LrgRoom.label points into it) and the filled-label arena of the same layout
    int32_t *fill_out_base;
    int fill_wgs;                // the last team of the first fill_wgs worker workgroups serves the fill-in ring only
    int small_teams;             // the first so many teams of a worker workgroup run branch tiles only, on the smaller LDS region (four teams per workgroup)
    int small_alt;               // 1: ... and one more of them on the odd workgroups
    int fill_extra;              // 1: ... and that team is one more than the other workgroups have (where LDS and threads allow: up to three tile teams)
    int fill_hybrid;             // 1: four tile teams per CU, the fill-in team is one of them: it takes a fill-in task when one is waiting and ring 1's next task otherwise
    // Shared tail tiles (nullable: tail == nullptr -> every slot pads its own last tile).  A slot's rows beyond its last full 32-row tile -- 16 of 91 rows per side
    // on average: 18 % of all tile rows were such padding -- are reserved from a cursor per side in rows that all slots share (LrgFrontArgs.tail_*), so that the
    // tails of several slots fill one BRANCH tile: the tile code's packed form (runs of rows of one slot each: per-run max-pool, lrg_forward_packed's arithmetic bit
    // for bit).  A tile is published by whoever brings its count of written rows to 32; a slot whose last tile stays open longer than tail_ticks closes it (the
    // cursor is moved to the tile's end, the missing rows count as dead).  The HEAD stack of a tail stays a tile of the slot's own: it reads the slot's conv[1] rows
    // where the shared tile left them and stores the logits of the slot's rows only (lrg_fused_tile: nrows_out).
    int32_t *tail;               // [0] / [16] the sides' row cursors (= LrgFrontArgs.tail_cur); [32 + side * tail_tiles + tile] rows accounted for | dead rows << 16
    int tail_tiles;              // shared tiles per side
    int tail_heads;              // 1 (without the units): the HEAD stacks of the tails run on the shared tiles too -- a shared tile's head task is published when the
                                 // pooled products of ALL slots with rows in it are complete ([32 + 2 * tail_tiles + side * tail_tiles + tile]: slots ready | the
                                 // tile's slots << 16); 0: a head tile of the slot's own per tail, storing its rows only
    long long tail_ticks;        // (wall_clock64: 100 MHz)
    float *pool_rows;            // nullable (with the units): [n_slots][2 sides][16 tiles][P / 2] column maxima by branch tile, instead of atomicMax on the pooled feature
    int pool_rows_stride;        // 2 * 16 * (P / 2)
    int poll_sleep;              // s_sleep(8) repeats between two polls of an idle team (1 = ~0.25 us)
    int branch_parts;            // tasks per branch tile (1, 2, 4): they share the column blocks of the pooled layer (lrg_fused_tile)
    // Wave-branch mode (round 6; lrg_wave_tile.inl): the launch is TWO kernels resident together -- lrg_grow_async_kernel with the front workgroups and the
    // pooled-product units only, and lrg_grow_async_worker_kernel (512 threads, up to 256 VGPRs) with `wave_wgs` wave-branch CUs and the head teams' CUs behind them.
    // A branch tile is a PREFIX task (layers 0 - 3, by one wavefront of a CU that holds those kernels of both branches in LDS) that publishes the tile's POOL tasks
    // (a quarter of the pooled layer each -- or half a quarter: wave_split 4 / 8 -- by one wavefront of a CU that holds its (side, half) of that kernel in LDS).
    // Rings of their own: 0 .. 3 = POOL tasks of (side, half), 4 = PREFIX tasks.  0: off -- one kernel, branch tiles by the tile teams.
    int wave_wgs;                // wave-branch CUs: workgroups 0 .. wave_a_wgs - 1 of the worker kernel run PREFIX tasks, wave_a_wgs .. wave_wgs - 1 POOL tasks of
    int wave_a_wgs;              //   (side, half) = (w - wave_a_wgs) & 3
    int wave_waves;              // wavefronts per wave-branch CU that run branch tasks (4: one per SIMD)
    int wave_split;              // POOL tasks per tile: 4 (a quarter = two pairs of column blocks each) or 8 (one pair each)
    int wave_fill;               // 1: wavefronts 4 .. 7 of the first fill_wgs wave-branch CUs are a fill-in team (VALU work beside the MFMA-bound branch waves)
    int wmask;                   // entries of one wave ring - 1 (power of two)
    float *h3[2];                // [row_cap, 128] per side: layer 3's output rows, from the PREFIX to the POOL tasks
    int rt_bb_every;             // register tiles: every so-manyth worker CU runs branch tiles on BOTH its teams (0: none)
    int rt_head_every;           // register tiles, CUs by role (lrg_rt_role below): of every so many CUs of an XCD's share of the worker grid one runs head tiles on both
                                 // teams, the others branch tiles on team 0 alone (0: none; never beside rt_bb_every)
    int unit_pairs;             // 1: the pooled-product units run their tasks on half-teams of two wavefronts (lrg_async_gemv_unit2)
    int unit_regs;               // 1: the pooled-product units keep their slice in registers and stream the rows through an LDS FIFO (lrg_async_gemv_unit3); before unit_pairs
    int reg_tiles;               // 1: the worker kernel's workgroups are all alike -- team 0 runs the branch tiles of ring 0 as REGISTER TILES (lrg_team_branch_tile_reg: a team
                                 // of four wavefronts per tile, layers 0 - 2 per wavefront in registers, one barrier), team 1 the pooled blocks and head tiles of ring 1
                                 // -- unless the CUs have roles (rt_bb_every, rt_head_every: lrg_rt_role below)
    int worker_base;             // blockIdx.x of the first worker workgroup in the kernel that runs the tile teams (n_front + gemv_units, or wave_wgs in the worker kernel)
    int total_wgs;               // workgroups of the launch in all (both kernels): what the start rendezvous waits for
    int max_steps;               // evaluations per slot in this launch
    long long start_ticks;       // ... the front workgroups wait at most this long for all workgroups of the launch to have started (reason 6)
    long long budget_ticks;      // wall_clock64 ticks (100 MHz) after which no new evaluation is started
    long long abort_ticks;       // ... after which a waiting workgroup gives up
    unsigned long long *work;    // nullable: [4] evaluations, distinct inlier rows, distinct neighbour rows, 32-row tiles (x 2 stacks) of this buffer's launches
    unsigned long long *dbg;     // nullable: [32] accumulators of wall-clock ticks (10 ns) for tools/free_run_perf.py --
                                 // 0 front busy, 1 front steps; per evaluation, since its tasks were published: 2 last branch tile in,
                                 // 3 last pooled-product block in, 4 last head tile in, 5 seen by the front workgroup, 6 evaluations;
                                 // 8 + 2 t busy ticks of task type t, 9 + 2 t their number; 16 ticks teams waited for a task, 17 waits;
                                 // the prepared mask update: 7 ticks spent making records, 19 records tried, 18 front steps that used one
};

// ---- the roles of a register-tile CU (LrgAsyncArgs.reg_tiles) ----
// Which ring's tickets the two teams of worker workgroup w take.  The matrix pipe is per SIMD and the two teams' wavefronts sit two to a SIMD: a head tile's MFMAs
// come straight out of the branch tile beside it.  By role a branch tile has its SIMDs to itself and head tiles share theirs with head tiles.
//   MIXED    team 0 branch tiles (ring 0), team 1 head tiles (ring 1)
//   BRANCH2  both teams branch tiles                                       (rt_bb_every)
//   BRANCH1  team 0 branch tiles, team 1's wavefronts leave at the start   (rt_head_every: the CUs that are not HEAD2)
//   HEAD2    both teams head tiles, no branch kernels in LDS               (rt_head_every)
// The worker grid goes round the 8 XCDs workgroup by workgroup, whichever XCD the round starts on: w / 8 counts the CUs of one XCD's share, so picking by it
// gives every XCD the same mix (and every XCD's L2 the kernels of both roles).  The one definition: the worker kernel (lrg_async.inl) and the host's table
// (tools/async_plan_table.hip --roles) both read it.
enum LrgRtRole { LRG_RT_MIXED = 0, LRG_RT_BRANCH2 = 1, LRG_RT_BRANCH1 = 2, LRG_RT_HEAD2 = 3 };
__host__ __device__ inline int lrg_rt_role(int w, int rt_bb_every, int rt_head_every) {
    if (rt_head_every > 0) return (w >> 3) % rt_head_every == rt_head_every - 1 ? LRG_RT_HEAD2 : LRG_RT_BRANCH1;
    if (rt_bb_every > 0 && w % rt_bb_every == rt_bb_every - 1) return LRG_RT_BRANCH2;
    return LRG_RT_MIXED;
}
// the ring team t (0, 1) of a CU of that role serves; -1: the team leaves
__host__ __device__ inline int lrg_rt_team_ring(int role, int t) {
    if (t == 0) return role == LRG_RT_HEAD2 ? 1 : 0;
    return role == LRG_RT_BRANCH2 ? 0 : role == LRG_RT_BRANCH1 ? -1 : 1;
}

// ---- the launch's arguments ----
// ONE kernel parameter, so that every role below can be a function of its own (own register allocation: the tile code needs 112
// VGPRs, a 1024-thread workgroup has 128 per lane -- inlined into one kernel body, the three task types and the front spilled
// ~150 dwords per lane, some of them inside the tiles' passes) and still reads the arguments the way a kernel does: scalar loads
// from the kernarg segment, nothing passed on, nothing copied to the stack.
struct LrgAsyncKArgs {
    LrgSlot *slots;
    LrgRoom *rooms;
    LrgGrowParams prm;
    LrgAsyncArgs A;
};

// The free-running launch's switches (A/B runs and test hooks; none changes a label), read from the environment on every call.
// The shape of a launch that the Python host chooses -- front workgroups, teams, units, parts, CUs, fill-in workgroups, branch_waves -- is set in LrgAsyncBuffers.
struct LrgAsyncSwitches {
    int unit_pairs;              // LRG_ASYNC_UNIT_PAIRS: 0 / non-zero forces the units' half-teams off / on; unset: on from 84 slots (never on unless the pooled feature has 1024 columns)
    int unit_regs;               // LRG_ASYNC_UNIT_REGS: 0 / non-zero forces the units' register form off / on; unset: see plan_units (never on unless the heads are the paper's: 1024 pooled features, 256 columns)
    int gemv_batch;              // LRG_ASYNC_GEMV_BATCH: > 0 batched pooled products where they fit (a launch without units); -1: off
    double gemv_batch_us;        // LRG_ASYNC_GEMV_BATCH_US: how long a batch waits for more slots, in us; 1.5
    int tail_heads;              // LRG_ASYNC_TAIL_HEADS: 0 = a head tile of the slot's own per tail; 1: the heads of the tails on the shared tiles too
    int rt_bb_every;             // LRG_ASYNC_RT_BB_EVERY: every so-manyth register-tile CU runs branch tiles on both teams (0: none); unset: 4 from 120 slots, else 0
    int rt_head_every;           // LRG_ASYNC_RT_HEAD_EVERY: register-tile CUs by role -- one CU in so many (per XCD) runs head tiles on both teams, the others branch tiles on one
                                 // (0: none, every CU mixed); a non-zero value turns rt_bb_every off; unset: see plan_two_kernels
    int wave_fronts;            // LRG_ASYNC_WAVE_FRONTS: > 0 front workgroups of a two-kernel launch; 0: as many as the shader engines they claim have room for
    int wave_extra_wgs;          // LRG_ASYNC_WAVE_EXTRA_WGS: (test hook) worker workgroups beyond what the shader engines hold; 0
    int wave_wgs;                // LRG_ASYNC_WAVE_WGS: > 0 wave-branch CUs; 0: 62 % (with units) | 55 % of the worker CUs
    int wave_a_wgs;              // LRG_ASYNC_WAVE_A_WGS: > 0 PREFIX CUs among them; 0: a fifth
    int wave_split;              // LRG_ASYNC_WAVE_SPLIT: 8 = a wave-branch tile as eight tasks; 0: four
    int rt_team_heads;           // LRG_ASYNC_RT_TEAM_HEADS: non-zero = register branch tiles with team head tiles; 0
    int fill_hybrid;             // LRG_ASYNC_FILL_HYBRID: 0 = a fourth team's fill-in team serves the fill-in ring only; 1: ring 1 too while no fill-in waits
    int ring0_halves;            // LRG_ASYNC_RING0_HALVES: > 0 half-teams per worker workgroup on branch tiles, -1 = one ring; 0: 3 with three teams or more, else 2
    int small_teams;             // LRG_ASYNC_SMALL_TEAMS: with four teams, 3 = three branch-only teams, 23 = 2 / 3 on even / odd workgroups; 0: two
};

// A free-running launch as lrg_async_plan decides it and async_launch carries it out
struct LrgAsyncPlan {
    LrgAsyncKArgs K;             // the front kernel's arguments (the worker kernel's: the same but for worker_base)
    bool two_kernels;            // the worker kernel on the side stream beside the front kernel
    int front_wgs;               // workgroups of the front kernel (the one-kernel launch: every CU it may use)
    int worker_wgs;              // workgroups of the worker kernel
    size_t lds, worker_lds;      // the two kernels' dynamic LDS
    int need_cus;                // the CUs the caller's stream must be allowed
    size_t tail_ctl_bytes;       // the shared tail tiles' control words, zeroed before the launch (0: no shared tail tiles)
};
// The switches as the environment sets them now (lrg_grow_async reads them on every call)
LrgAsyncSwitches lrg_async_switches();
// The tests of lrg_grow_async's arguments that need nothing but the arguments: 0, or the LRG_EINVAL code lrg_grow_async returns
int lrg_async_check(LrgSlot *slots, LrgRoom *rooms, int n_slots, int max_points, const LrgGrowParams *params, const LrgWeights *weights,
                    const LrgPackedBuffers *b, const LrgAsyncBuffers *ab, int max_steps, int budget_us);
// The launch's shape from arguments that passed lrg_async_check, the device's CU count and the switches -- no HIP call, no state, no pointer dereferenced but
// params, weights, b and ab: 0 and *plan, or the LRG_EINVAL code lrg_grow_async returns
int lrg_async_plan(LrgSlot *slots, LrgRoom *rooms, int n_slots, int max_points, const LrgGrowParams *params, const LrgWeights *weights,
                   const LrgPackedBuffers *b, const LrgAsyncBuffers *ab, int max_steps, int budget_us, int cus, const LrgAsyncSwitches &sw,
                   LrgAsyncPlan *plan);
// The shape of the process's last lrg_grow_async launch, for tests and tools (not part of include/lrg_hip.h): up to LRG_ASYNC_LAST_PLAN_WORDS words --
// [0] 1 once a launch was planned, [1] two_kernels, [2] front_wgs, [3] worker_wgs, [4] n_front, [5] gemv_units, [6] unit_pairs, [7] unit_regs, [8] reg_tiles,
// [9] teams, [10] per-tile pool rows in use, [11] n_slots.  Returns the words written.
#define LRG_ASYNC_LAST_PLAN_WORDS 12
extern "C" int lrg_async_last_plan(int32_t *out, int n);
