// The host side of the free-running launch (lrg_grow_async): the sizes of its buffers, its switches, the checks of its arguments, the launch plan and the launch.
// Included by lrg_grow.hip behind the device code (lrg_front.inl, lrg_async.inl, lrg_wave_tile.inl), whose LDS-size macros the plan needs; the structs and the
// three functions that tools/async_plan_table.hip calls are declared in lrg_async_plan.h.

static size_t async_ring_entries(int n_slots) {
    size_t ring = 1 << 14;                                   // entries: far more than the tasks that can be outstanding (~80 per slot)
    while (ring < (size_t)n_slots * 512) ring <<= 1;
    return ring;
}
static size_t async_unit_ring_entries(int n_slots) {         // the pooled-product units' ring: a slot has one entry outstanding at most -- and with batched pooled
    size_t ring = 256;                                       // products (LRG_GEMV_BATCH) a closed batch takes LRG_GEMV_BATCH positions whatever it holds: live batches
    while (ring < (size_t)n_slots * 2 * LRG_GEMV_BATCH) ring <<= 1;      // span up to LRG_GEMV_BATCH x n_slots positions (twice that: nobody wraps onto an unread entry)
    return ring;
}
static size_t async_wave_ring_entries(int n_slots) {         // one of the eight (side, quarter) rings of a wave-branch launch: a slot has at most 16 tiles per side outstanding
    size_t ring = 2048;
    while (ring < (size_t)n_slots * 32) ring <<= 1;
    return ring;
}
size_t lrg_grow_async_queue_bytes(int n_slots) {
    if (n_slots <= 0) return 0;
    // (two task rings: branch tiles | pooled blocks and head tiles; then the units' ring; then the fill-in ring; then the wave rings' control words and the eight wave rings)
    return (LRG_AQ_RING + 2 * async_ring_entries(n_slots) + async_unit_ring_entries(n_slots) + LRG_ASYNC_FILL_RING + 256 + 8 * async_wave_ring_entries(n_slots)) * sizeof(int32_t);
}

// the network lrg_wave_tile.inl is written for: 9 .. 16 features, branch layers 64, 64, 64, 128, 512 and heads 256, 128, 2 (the LrgNet of the paper, lite 0).
// The heads too: lrg_team_head_tile_reg reads the pooled product at a stride of 256, 8 / 32 k-groups and a bias of 128 -- packed_shapes accepts other head stacks
// on the paper's branches, and those keep the one-kernel launch, whose team tiles are general.  The one test of the network that both async_reg_candidate and
// async_two_kernels_fit read, so that the units' slot limit follows the launch that is made.
static bool lrg_wave_branch_fits(const LrgWeights *w) {
    return w->feature_size > 8 && w->feature_size <= LRG_WB_K0 && w->n_conv == 5 && w->conv_ch[0] == LRG_WB_C0 && w->conv_ch[1] == LRG_WB_C1 && w->conv_ch[2] == LRG_WB_C2 &&
           w->conv_ch[3] == LRG_WB_C3 && w->conv_ch[4] == LRG_WB_C4 && w->n_head == 3 && w->head_ch[0] == 256 && w->head_ch[1] == 128 && w->head_ch[2] == 2;
}

// the side stream and the two events of a wave-branch launch (per device; created once)
// (a ring of event pairs: a launch's events are not recorded again while an earlier launch's waits on them may still be queued -- callers run a few launches ahead)
#define LRG_SIDE_EVENTS 64
struct LrgSideStream { hipStream_t stream; hipEvent_t start[LRG_SIDE_EVENTS], done[LRG_SIDE_EVENTS]; std::atomic<unsigned> next; bool ok; };
static LrgSideStream *lrg_side_stream() {
    static LrgSideStream side[LRG_MAX_DEVICES] = {};
    static std::mutex init;                                  // (host threads that launch at once: one of them creates the stream and events, the others wait for it)
    LrgSideStream *s = &side[lrg_current_device()];
    std::lock_guard<std::mutex> lock(init);
    if (!s->ok) {
        // HIP streams are mapped onto a few hardware queues (four per priority level), round robin by creation, and kernels of two streams that share a queue never run
        // side by side: with a side stream of the callers' own priority every fourth new caller stream landed on its queue -- the worker kernel waited out its 4 s for a
        // front kernel queued BEHIND it (3 of 12 growers, tools/r06_spec_soak.py).  The side stream is created at the HIGHEST priority: a queue of another pool than any
        // stream of default priority.  (A caller that launches from a highest-priority stream of its own can still collide: found out by the start rendezvous, reason 6 / 2.)
        int prio_least = 0, prio_greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
        if (hipStreamCreateWithPriority(&s->stream, hipStreamNonBlocking, prio_greatest) != hipSuccess) return nullptr;
        for (int i = 0; i < LRG_SIDE_EVENTS; ++i)
            if (hipEventCreateWithFlags(&s->start[i], hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&s->done[i], hipEventDisableTiming) != hipSuccess) return nullptr;
        s->ok = true;
    }
    return s;
}

size_t lrg_grow_async_tail_bytes(int n_slots, int tail_rows) {
    if (n_slots <= 0 || tail_rows <= 0 || (tail_rows & 31)) return 0;
    // (the two row cursors on a 64-byte line each, two words per shared tile and side, the slots' tail bases)
    return (size_t)(32 + 4 * (size_t)(tail_rows / 32) + 2 * (size_t)n_slots) * sizeof(int32_t);
}

size_t lrg_grow_async_pool_rows_bytes(const LrgWeights *weights, int n_slots) {
    if (!weights || n_slots <= 0 || weights->n_conv < 1) return 0;
    return (size_t)n_slots * 2 * 16 * (size_t)weights->conv_ch[weights->n_conv - 1] * sizeof(float);      // [slot][side][tile][columns of the pooled layer]
}

// The switches (LrgAsyncSwitches, lrg_async_plan.h) as the environment sets them at this call
LrgAsyncSwitches lrg_async_switches() {
    LrgAsyncSwitches s;
    s.unit_pairs = lrg_env_int("LRG_ASYNC_UNIT_PAIRS", LRG_ENV_UNSET);
    s.unit_regs = lrg_env_int("LRG_ASYNC_UNIT_REGS", LRG_ENV_UNSET);
    s.gemv_batch = lrg_env_int("LRG_ASYNC_GEMV_BATCH", -1);
    s.gemv_batch_us = lrg_env_real("LRG_ASYNC_GEMV_BATCH_US", 1.5);
    s.tail_heads = lrg_env_int("LRG_ASYNC_TAIL_HEADS", 1);
    s.rt_bb_every = lrg_env_int("LRG_ASYNC_RT_BB_EVERY", LRG_ENV_UNSET);
    s.rt_head_every = lrg_env_int("LRG_ASYNC_RT_HEAD_EVERY", LRG_ENV_UNSET);
    s.wave_fronts = lrg_env_int("LRG_ASYNC_WAVE_FRONTS", 0);
    s.wave_extra_wgs = lrg_env_int("LRG_ASYNC_WAVE_EXTRA_WGS", 0);
    s.wave_wgs = lrg_env_int("LRG_ASYNC_WAVE_WGS", 0);
    s.wave_a_wgs = lrg_env_int("LRG_ASYNC_WAVE_A_WGS", 0);
    s.wave_split = lrg_env_int("LRG_ASYNC_WAVE_SPLIT", 0);
    s.rt_team_heads = lrg_env_int("LRG_ASYNC_RT_TEAM_HEADS", 0);
    s.fill_hybrid = lrg_env_int("LRG_ASYNC_FILL_HYBRID", 1);
    s.ring0_halves = lrg_env_int("LRG_ASYNC_RING0_HALVES", 0);
    s.small_teams = lrg_env_int("LRG_ASYNC_SMALL_TEAMS", 0);
    return s;
}

static int async_row_stride(const LrgGrowParams *params) { return (max(params->n_inlier, params->n_neighbor) + 31) / 32 * 32; }

// The tests that need nothing but the arguments (the codes of those that need derived values are returned by lrg_async_plan)
int lrg_async_check(LrgSlot *slots, LrgRoom *rooms, int n_slots, int max_points, const LrgGrowParams *params, const LrgWeights *weights,
                    const LrgPackedBuffers *b, const LrgAsyncBuffers *ab, int max_steps, int budget_us) {
    int rc = check_params(params);
    if (rc) return rc;
    if (!slots || !rooms || !weights || !b || !ab || n_slots <= 0 || max_points <= 0 || max_steps < 1 || budget_us < 0) return LRG_EINVAL - 1;
    if (weights->feature_size != params->feature_size) return LRG_EINVAL - 2;
    if (!lrg_uses_greedy_front(params, b) || max_points > LRG_FRONT_MAXCHUNK * LRG_SCAN_CHUNK) return LRG_EINVAL - 3;
    if (!b->center || !b->sample_in || !b->sample_nb || !b->x_in || !b->x_nb || !b->row_slot_in || !b->row_slot_nb || !b->upd_in ||
        !b->upd_nb || !b->rmv_logits || !b->add_logits || !b->slot_rows || !b->counters || !b->workspace || !ab->queue || !ab->sync)
        return LRG_EINVAL - 4;
    if (b->row_cap % LRG_ROW_TILE != 0 || (long)b->row_cap < (long)n_slots * async_row_stride(params)) return LRG_EINVAL - 5;
    if (ab->queue_bytes < lrg_grow_async_queue_bytes(n_slots) || ((uintptr_t)ab->queue & 255) || n_slots >= (1 << 20)) return LRG_EINVAL - 6;
    return 0;
}

// Whether this launch takes register tiles (a two-kernel launch) is previewed here and decided later, and the two tests do not agree today (making them agree
// changes launches: left to a change of its own).
// async_reg_candidate: asked before the pooled-product units are decided, so that register-tile launches keep their units up to LRG_REG_TILE_AUTO_MAX slots.
// It looks at what was ASKED for: want == 1 (or 0 inside the automatic range), LrgAsyncBuffers.rows16, no shared tail tiles, no pool rows, the paper's network,
// the whole chip.
static bool async_reg_candidate(int want, int n_slots, const LrgAsyncBuffers *ab, const LrgWeights *weights, bool tails_on, int cus) {
    return (want == 1 || (want == 0 && n_slots >= LRG_REG_TILE_AUTO_MIN && n_slots <= LRG_REG_TILE_AUTO_MAX)) && ab->rows16 && !tails_on && !ab->pool_rows &&
           lrg_wave_branch_fits(weights) && !(ab->compute_units > 0 && ab->compute_units < cus);
}
// async_two_kernels_fit: whether a two-kernel launch (register tiles or wave-branch tasks) can be made, asked once the rest of the launch is decided.  Unlike the
// preview it looks at what was GRANTED -- rows at a 64-byte stride (which also needs 9 .. 16 features and aligned rows), no shared tail tiles, no pool rows, no
// batched pooled products -- and further at the branch problem's layers, a chip of whole shader engines (a multiple of 32, at least 64 CUs) and n_slots < 2^20;
// it does not look at `want`.
static bool async_two_kernels_fit(const LrgAsyncArgs &A, const LrgAsyncBuffers *ab, const LrgWeights *weights, int n_slots, int wgs, int cus) {
    return A.front.rows16 && !A.tail && !A.pool_rows && !A.gemv_batch && lrg_wave_branch_fits(weights) &&      // (batched pooled products: tasks of the one-kernel launch's teams)
           A.prob[0].nlayers == 5 && A.prob[0].L[1].gout && A.prob[0].pool &&
           (ab->compute_units <= 0 || ab->compute_units >= cus) && (wgs % 32) == 0 && wgs >= 64 && n_slots < (1 << 20);
}

// ---- The launch plan ----
// lrg_async_plan below is a sequence of steps, in the order that fixes which error code wins.  A step's parameters say what it reads -- the caller's arguments, the
// switches, earlier decisions by value -- and what it decides: the fields it writes through its pointers (named in its comment) and the code it can return.
// Every launch the steps decide is pinned by tests/golden/async_plan_table.txt (tools/async_plan_table.hip): a change to a decision shows there as the rows it moves.

// (1) The four problems and the pooled product as lrg_forward_packed would launch them, and the shapes the team tiles are instantiated for (LRG_EINVAL - 7)
static int plan_problems(const LrgWeights *weights, const LrgPackedBuffers *b, int n_slots, LrgFusedProb prob[4], LrgGemvArgs *gemv) {
    LrgFusedArgs branches, heads;
    int rc = lrg_packed_problems(weights, b->x_in, b->x_nb, b->center, b->row_slot_in, b->row_slot_nb, b->counters, n_slots, b->row_cap,
                                 b->add_logits, b->rmv_logits, b->workspace, b->workspace_bytes, &branches, gemv, &heads);
    if (rc) return rc;
    prob[0] = branches.p[0]; prob[1] = branches.p[1]; prob[2] = heads.p[0]; prob[3] = heads.p[1];
    for (int i = 0; i < 4; ++i) {
        const LrgFusedProb &P = prob[i];
        // the shapes the team tiles are instantiated for: lite 0 / 2 (lite 1 stores conv[1] from the accumulators: lrg_grow_step_packed)
        const int Kp = (P.Kin + 7) & ~7;
        if (32 * (Kp + 4) > (i < 2 ? 32 * 132 : 32 * 68)) return LRG_EINVAL - 7;
        for (int l = 0; l < P.nlayers; ++l) {
            const LrgFusedLayer &L = P.L[l];
            const bool inplace = (L.flags & LRG_FL_INPLACE) != 0, to_buf1 = ((l & 1) != 0) == !inplace;
            if (L.gout && (!(L.flags & LRG_FL_KEEP) || inplace)) return LRG_EINVAL - 7;
            if ((L.flags & LRG_FL_KEEP) && 32 * (L.N + 4) > (to_buf1 ? (i < 2 ? 32 * 132 : 32 * 68) : (i < 2 ? 32 * 68 : 32 * 260))) return LRG_EINVAL - 7;
        }
    }
    if (gemv->P + 8 * LRG_GEMV_TASK_COLS > LRG_ASYNC_TILE_FLOATS || (gemv->P & 127) || (gemv->ldw & 3) || (gemv->C & 3) ||
        (((uintptr_t)gemv->w[0] | (uintptr_t)gemv->w[1]) & 15))
        return LRG_EINVAL - 7;                              // (pooled product: sixteen 16-byte rows in flight per lane, K ranges of P / 8)
    return 0;
}

// (2) The front's arguments.  Decides a->rows16, and with it the stride the branch problems read their rows at (prob[0 .. 1].ldx).
static int plan_front_args(const LrgGrowParams *params, const LrgWeights *weights, const LrgPackedBuffers *b, const LrgAsyncBuffers *ab, int n_slots, int row_stride,
                           LrgFrontArgs *a, LrgFusedProb prob[4]) {
    int rc = lrg_front_args(weights, b, n_slots, a);
    if (rc) return rc;
    a->phase_ticks = nullptr;
    a->own_medians = 1; a->row_stride = row_stride;
    a->rows16 = 0;
    if (ab->rows16 && params->feature_size > 8 && (((uintptr_t)b->x_in | (uintptr_t)b->x_nb | (uintptr_t)b->center) & 15) == 0) {
        // the caller's row arrays hold row_cap x 16 floats: gathered rows at a 64-byte stride, written and read in 16-byte pieces (9 .. 16 features)
        a->rows16 = 1;
        prob[0].ldx = 16; prob[1].ldx = 16;
    }
    a->phase_dbg = ab->debug_ticks ? reinterpret_cast<unsigned long long *>(ab->debug_ticks) + 20 : nullptr;
    return 0;
}

// (3) The CUs in use (*wgs), whether shared tail tiles were asked for (*tails_on) and the front workgroups (*n_front); LRG_EINVAL - 8
static int plan_front_workgroups(const LrgAsyncBuffers *ab, int n_slots, int cus, int *wgs_out, bool *tails_on_out, int *n_front_out) {
    int wgs = cus;
    if (ab->compute_units > 0 && ab->compute_units < wgs) wgs = ab->compute_units;
    // Front workgroups: one per two slots (a front step takes ~23 us of a ~85 us step, and a CU a front workgroup holds is a CU without
    // tile teams: 68 slots, two teams: 34 / 40 / 46 / 68 front workgroups 806 / 810 / 807 / 792 k instance-steps/s, profiles/r03_units_sweep.log);
    // one per slot while the slots are few and CUs plenty (eight 100 k-point scenes: 8 / 4 front workgroups 97 k / 86 k, profiles/r03_kitti2_*.json)
    // ... and never more than an eighth of the CUs (+ 2: 34 of 256) by default: a front step takes ~24 us whatever the number of slots, so
    // ~1 M steps/s keep ~25 front workgroups busy, and every CU beyond that is a CU without tile teams (192 slots: 24 / 28 / 34 / 48 front
    // workgroups 0.92 / 1.06 / 1.17 / 1.11 M instance-steps/s; 272 slots: 34 / 40 / 48 / 64 / 96: 1.11 / 1.07 / 1.02 / 0.94 / 0.76 M)
    // (with shared tail tiles -- a sixth fewer branch tiles -- the tile teams need fewer CUs and the slots more: 272 slots 34 / 40 / 46 / 52 front workgroups
    //  828 (without them) / 872 / 871 / 858 rooms/s, 320 slots 40 / 44 / 48: 876 / 886 / 881, profiles/r05_tail_fronts*.txt)
    const bool tails_on = ab->tail_ctl && ab->tail_rows > 0 && ab->rows16 && !ab->pool_rows;
    int n_front = ab->front_workgroups > 0 ? ab->front_workgroups : n_slots <= 24 ? n_slots : min((n_slots + 1) / 2, tails_on ? wgs * 11 / 64 : wgs / 8 + 2);
    n_front = min(n_front, n_slots);
    n_front = max(n_front, (n_slots + LRG_ASYNC_MAX_SERVED - 1) / LRG_ASYNC_MAX_SERVED);
    n_front = min(n_front, wgs / 2);                         // (at least half of the CUs for the tile teams)
    if (n_front < (n_slots + LRG_ASYNC_MAX_SERVED - 1) / LRG_ASYNC_MAX_SERVED) return LRG_EINVAL - 8;      // more slots than the front workgroups can serve
    *wgs_out = wgs; *tails_on_out = tails_on; *n_front_out = n_front;
    return 0;
}

// (4) Speculation (LrgAsyncBuffers.speculate = K > 1): groups of K slots on one room each, one front workgroup per group (a group's shared state -- the
// room's visited flags, labels, seed cursor, the other slots' boxes -- stays on one CU and needs no hand-over).
// Decides a->spec_k, a->spec_stats and, with speculation on, *n_front; LRG_EINVAL - 8
static int plan_speculation(const LrgAsyncBuffers *ab, int n_slots, int wgs, LrgFrontArgs *a, int *n_front) {
    a->spec_k = 0;
    a->spec_stats = nullptr;
    if (ab->speculate > 1) {
        if (ab->speculate > LRG_ASYNC_MAX_SERVED || n_slots % ab->speculate != 0 || n_slots / ab->speculate > wgs / 2) return LRG_EINVAL - 8;
        a->spec_k = ab->speculate;
        *n_front = n_slots / ab->speculate;
        if (ab->work) a->spec_stats = reinterpret_cast<unsigned long long *>(ab->work) + 4;
    }
    return 0;
}

// (5) Pooled-product units (lrg_async.inl): sixteen CUs for the LrgNet of the paper (2 heads x 256 columns, 1024 pooled features).
// Off (-1), or where the slices do not fit / would leave the tile teams fewer than half of the CUs: the teams' 128-column blocks.  Off
// above 176 slots too: sixteen units take ~1.1 M pooled products a second, and the head tiles that wait for them hold their teams
// (136 / 160 / 192 / 272 slots with | without units: 1.13 | 1.03, 1.15 | 1.11, 1.14 | 1.17, 1.06 | 1.11 M instance-steps/s, profiles/r03_slots_sweep.log;
//  end of round 4, profiles/r04_teams_units_sweep.txt: 136 / 160 / 176 slots 1.15 | 1.09, 1.16 | 1.19, 1.17 | 1.23 M -- off above 148).
// Decides A->gemv_units, unit_pairs, gemv_batch, gemv_batch_ticks.
static void plan_units(const LrgAsyncBuffers *ab, const LrgWeights *weights, const LrgAsyncSwitches &sw, const LrgGemvArgs &g, int n_slots, int cus, int wgs,
                       bool tails_on, int n_front, LrgAsyncArgs *A) {
    int units = (g.C % LRG_GEMV_UNIT_COLS == 0) ? 2 * g.C / LRG_GEMV_UNIT_COLS : 0;
    // (register-tile launches keep the units up to their last slot count: 160 slots with units and every fourth worker CU on two branch teams 1.26 M against 1.20 M
    //  instance-steps/s for the one-kernel launch without units, profiles/r06_reg_tiles_slots.txt)
    const bool reg_candidate = async_reg_candidate(ab->branch_waves, n_slots, ab, weights, tails_on, cus);
    if (ab->gemv_units < 0 || (ab->gemv_units == 0 && n_slots > (reg_candidate ? LRG_REG_TILE_AUTO_MAX : 148)) || (size_t)max((int)LRG_GEMV_UNIT_FLOATS(g.P), (int)LRG_GEMV_UNIT2_FLOATS(g.P)) * sizeof(float) + 16 > 160 * 1024 || n_slots > LRG_GEMV_UNIT_MAX_SLOTS || (((uintptr_t)g.pooled) & 15) ||
        n_front + units > wgs / 2 + wgs / 4)
        units = 0;
    A->gemv_units = units;
    // (half-teams in the units, lrg_async_gemv_unit2: eight tasks in flight per unit, each a little longer.  68 / 100 / 136 slots with register tiles: 992 -> 975,
    //  1 147 -> 1 189, 1 156 -> 1 206 k instance-steps/s (profiles/r06_unit_pairs.txt): on from 84 slots, where the units' capacity is what a slot queues for;
    //  LRG_ASYNC_UNIT_PAIRS=0 / 1 forces)
    // ... of the paper's 2 x 512 pooled features only, forced or not: lrg_async_gemv_unit2 fetches a slot's row as two loads of 512 floats and stages half a row of
    // P / 2 = 512 -- lite 2 (P = 512) keeps the four-wavefront units, which are general in P
    const bool pairs_fit = g.P == 1024;
    A->unit_pairs = !pairs_fit ? 0 : sw.unit_pairs != LRG_ENV_UNSET ? (sw.unit_pairs ? 1 : 0) : (units && n_slots >= 84 ? 1 : 0);
    // (the slice in registers, lrg_async_gemv_unit3: the kernel prefers it over the half-teams, whose field keeps its value.  For the paper's heads only -- 64 weights
    //  a lane are a [1024, 32] slice on eight wavefronts -- and where its FIFO fits the units' LDS, which it does not enlarge; LRG_ASYNC_UNIT_REGS=0 / 1 forces.
    //  The figures behind the default: profiles/unit_registers.txt)
    const bool regs_fit = units && g.P == LRG_GEMV_UNIT3_P && g.C == 256 &&
                          (size_t)LRG_GEMV_UNIT3_FLOATS * sizeof(float) <= (size_t)max((int)LRG_GEMV_UNIT_FLOATS(g.P), (int)LRG_GEMV_UNIT2_FLOATS(g.P)) * sizeof(float) + 16;
    A->unit_regs = !regs_fit ? 0 : sw.unit_regs != LRG_ENV_UNSET ? (sw.unit_regs ? 1 : 0) : 1;
    // without the units: the pooled products in batches (lrg_async.inl, LRG_GEMV_BATCH) where slots become ready faster than a batch's patience --
    // LRG_ASYNC_GEMV_BATCH=0 / =1: off / on whatever the slot count; LRG_ASYNC_GEMV_BATCH_US: the patience
    const int batch_us10 = (int)(10.0 * sw.gemv_batch_us);
    const bool fits = (size_t)(LRG_GEMV_BATCH * (g.P + 4)) <= (size_t)LRG_ASYNC_TILE_FLOATS && g.P == 1024 && (g.C & 31) == 0 && n_slots < LRG_GEMV_NOBODY;      // (half ranges of eight k-groups: the paper's 2 x 512 pooled features)
    // (2 176 room jobs, rooms/s without | with: 200 slots 771 | 731, 272: 873 | 800, 320: 888 | 850, 400: 880 | 896 -- a block takes 68 us for ~7.7 slots instead
    //  of 23 us for one, 35 instead of 93 team-us per evaluation, but the pooled stage of a slot's step grows from 71 to 108 us and below ~400 slots the launch is
    //  bound by that latency, not by its teams: profiles/r05_gemv_batch_v1.txt, r05_bench_debug_batch.log)
    // ... and the matrix-core form of the block (this build): 200 slots 773 | 723, 272: 871 | 791, 320: 885 | 837, 400: 884 | 877; with shared head tiles 400: 884-911 | 864,
    // 544: 906 | 905 (profiles/r05_gemv_batch_v3_mfma_pipelined.txt, r05_tail_heads2.txt).  The block for one slot costs the tile teams' CU nothing but L2 latency
    // (its few FMAs run beside the other teams' MFMAs); the batch's block costs matrix-pipe time -- 32-row tiles for ~8 slots -- which is what the launch is short of.
    // Off unless asked for (LRG_ASYNC_GEMV_BATCH=1).
    A->gemv_batch = (units == 0 && fits && sw.gemv_batch > 0) ? LRG_GEMV_BATCH : 0;
    A->gemv_batch_ticks = (long long)batch_us10 * 10;
}

// (6) In-launch fill-in (lrg_async.inl): the caller's arenas for the lists of unlabeled points and the best (distance, index) words, laid out like
// the label arena; 13 features (the compiled-in search); one team each of up to sixteen worker workgroups serves the fill-in ring.
// Decides A->fill_list, fill_best, fill_sync, fill_label_base, fill_out_base (the fill-in teams: step 10) and a->fill_in_launch; LRG_EINVAL - 6
static int plan_fill_buffers(const LrgAsyncBuffers *ab, const LrgGrowParams *params, int max_points, LrgAsyncArgs *A, LrgFrontArgs *a) {
    A->fill_list = nullptr; A->fill_best = nullptr; A->fill_sync = nullptr; A->fill_label_base = nullptr; A->fill_out_base = nullptr; A->fill_wgs = 0; A->fill_extra = 0; A->fill_hybrid = 0;
    a->fill_in_launch = 0;
    if (ab->fill_list && ab->fill_best && ab->fill_sync && ab->fill_label_base && ab->fill_out_base && params->feature_size == 13 && ab->fill_rooms > 0 &&
        ab->fill_rooms <= (1 << 18) && max_points <= 1024 * LRG_NN1_C) {
        if ((uintptr_t)ab->fill_best & 7) return LRG_EINVAL - 6;
        A->fill_list = ab->fill_list; A->fill_best = reinterpret_cast<unsigned long long *>(ab->fill_best); A->fill_sync = ab->fill_sync;
        A->fill_label_base = ab->fill_label_base; A->fill_out_base = ab->fill_out_base;
        a->fill_in_launch = 1;
    }
    return 0;
}

// (7) Shared tail tiles: the caller's row arrays continue behind the slots' own rows.
// Decides A->tail, tail_tiles, tail_ticks, tail_heads, a->tail_cur, tail_base, tail_rows, tail_row0 and *tail_ctl_bytes; LRG_EINVAL - 9
static int plan_tail_tiles(const LrgAsyncBuffers *ab, const LrgPackedBuffers *b, const LrgAsyncSwitches &sw, int n_slots, int row_stride, int rows16, int gemv_units,
                           LrgAsyncArgs *A, LrgFrontArgs *a, size_t *tail_ctl_bytes) {
    A->tail = nullptr; A->tail_tiles = 0; A->tail_ticks = 0; A->tail_heads = 0;
    *tail_ctl_bytes = 0;
    a->tail_cur = nullptr; a->tail_base = nullptr; a->tail_rows = 0; a->tail_row0 = 0;
    if (ab->tail_ctl && ab->tail_rows > 0 && rows16 && !ab->pool_rows) {
        // (+ 32 rows: a slot's own head tile on its tail rows stages a full tile from the tail's first row, tail_heads == 0)
        if ((ab->tail_rows & 31) || ((uintptr_t)ab->tail_ctl & 63) || (long)b->row_cap < (long)n_slots * row_stride + ab->tail_rows + 32 || ab->tail_rows / 32 >= (1 << 20))
            return LRG_EINVAL - 9;
        A->tail = ab->tail_ctl; A->tail_tiles = ab->tail_rows / 32;
        A->tail_ticks = ab->tail_close_us < 0 ? 0 : ab->tail_close_us > 0 ? (long long)ab->tail_close_us * 100 : 200;
        a->tail_cur = ab->tail_ctl; a->tail_rows = ab->tail_rows; a->tail_row0 = n_slots * row_stride;
        a->tail_base = ab->tail_ctl + 32 + 4 * (size_t)A->tail_tiles;
        // (the heads of the tails on the shared tiles too -- without the units, whose head tiles start before the pooled product is complete and wait inside;
        //  LRG_ASYNC_TAIL_HEADS=0: a head tile of the slot's own per tail)
        A->tail_heads = (gemv_units == 0 && sw.tail_heads != 0) ? 1 : 0;
        *tail_ctl_bytes = (32 + 4 * (size_t)A->tail_tiles) * sizeof(int32_t);
    }
    return 0;
}

// (8) Pool rows.  With the units, a branch tile leaves its column maxima of the pooled layer as one row of 16-byte stores (pool_rows) and the units take
// the maximum over a slot's tiles while loading: no atomicMax per column (7 k atomics = write transactions per evaluation, each to
// be acknowledged before the tile may report in), no zeroing of the pooled feature by the front workgroup.
// Decides A->pool_rows, pool_rows_stride, the branch problems' pool_rows and a->pooled; LRG_EINVAL - 6
static int plan_pool_rows(const LrgAsyncBuffers *ab, int n_slots, int row_stride, int gemv_units, int P, LrgAsyncArgs *A, LrgFrontArgs *a) {
    A->pool_rows = nullptr; A->pool_rows_stride = 0;
    if (gemv_units && ab->pool_rows && row_stride <= 512 && n_slots <= 4096) {
        const size_t need = (size_t)n_slots * 2 * 16 * (P / 2) * sizeof(float);
        if (ab->pool_rows_bytes < need || ((uintptr_t)ab->pool_rows & 15)) return LRG_EINVAL - 6;
        A->pool_rows = ab->pool_rows; A->pool_rows_stride = 2 * 16 * (P / 2);
        for (int side = 0; side < 2; ++side) {
            A->prob[side].pool_rows = ab->pool_rows + (size_t)side * 16 * (P / 2);
            A->prob[side].pool_rows_stride = A->pool_rows_stride;
        }
        a->pooled = nullptr;         // (nobody accumulates into it)
    }
    return 0;
}

// (9) Two-kernel launches (round 6, lrg_wave_tile.inl / lrg_grow_async_worker_kernel): the tile CUs as a second kernel of 512 threads and up to 256 VGPRs, resident
// beside the front workgroups' and units' kernel.  LrgAsyncBuffers.branch_waves: 1 = REGISTER TILES (a branch tile by a team of four wavefronts, layers 0 - 2 per
// wavefront in registers, one barrier: the default from LRG_REG_TILE_AUTO_MIN to LRG_REG_TILE_AUTO_MAX slots), 4 / 8 = one-wavefront PREFIX / POOL tasks on CUs that
// keep the kernels of their stage in LDS, -1 = one kernel.  Needs the rows at a 64-byte stride, the paper's network, no shared tail tiles / per-tile pool rows, and the
// whole chip (the two grids are sized per shader engine: a CU-masked launch keeps the one-kernel form).  The paper's network: its branches AND its heads 256, 128, 2
// (lrg_wave_branch_fits) -- any other head stack on the paper's branches keeps the one-kernel form, as lite 2 does.
// Reads what steps 1 - 8 left in *A (async_two_kernels_fit).  Decides A->wave_wgs, wave_a_wgs, wave_waves, wave_split, wave_fill, wmask, h3, reg_tiles, rt_bb_every,
// rt_head_every (as asked for: plan_roles grants it), may raise *n_front, and returns the worker kernel's workgroups (0: one kernel).
//
// Register-tile CUs by role (lrg_rt_role, lrg_async_plan.h; profiles/cu_roles.txt): of every 3 CUs of an XCD's share one runs head tiles on both teams, two run
// branch tiles on one team -- 128 branch-only and 64 head-only CUs of 192.  A branch tile beside a head team that never pauses takes 50.4 k ticks, alone 32.0 k; a
// head tile beside a head team 28.0 k, beside a branch team 36.2 k.  Plain benchmark, k instance-steps/s, every CU mixed | one in 3 (two runs each, no overlap up to
// 76): 4 slots 101 | 102, 8: 198 | 206, 16: 364 | 376, 24: 509 | 534, 34: 628 | 664, 46: 808 | 854, 52: 883 | 930, 60: 971 | 1 009, 68: 1 049 | 1 080,
// 72: 1 084 | 1 107, 76: 1 113 | 1 122, 80: 1 135 | 1 137, 84: 1 185 | 1 178, 92: 1 233 | 1 196, 100: 1 258 | 1 206, 136: 1 305 | 1 204, 160: 1 310 | 1 214 --
// beyond ~80 slots the 128 branch teams are what a slot's tiles queue for.  One in 2 (96 branch teams) loses from 52 slots (68: 912), one in 4 (96 head teams)
// at 68 (928).  Automatic from 4 to 72 slots, where it wins at every measured point by 2 % or more (4 slots: 1 %); elsewhere today's plan, rt_bb_every included.
#ifndef LRG_RT_HEAD_EVERY_AUTO
#define LRG_RT_HEAD_EVERY_AUTO(n_slots) ((n_slots) >= 4 && (n_slots) <= 72 ? 3 : 0)
#endif
static int plan_two_kernels(const LrgAsyncBuffers *ab, const LrgWeights *weights, const LrgPackedBuffers *b, const LrgAsyncSwitches &sw, int n_slots, int wgs, int cus,
                            LrgAsyncArgs *A, int *n_front_io) {
    A->wave_wgs = 0; A->wave_a_wgs = 0; A->wave_waves = 0; A->wave_split = 4; A->wave_fill = 0; A->wmask = (int)async_wave_ring_entries(n_slots) - 1; A->h3[0] = A->h3[1] = nullptr; A->reg_tiles = 0;
    // (every fourth register-tile CU with two branch teams from 120 slots: a slot's branch tiles queue for their teams there -- 68 slots -2.5 %, 100: +0.3 %, 136: +3.6 %, 160: +4.6 %)
    A->rt_bb_every = sw.rt_bb_every != LRG_ENV_UNSET ? sw.rt_bb_every : (n_slots >= 120 ? 4 : 0);
    // (register-tile CUs by role, lrg_rt_role: what is asked for -- plan_roles below grants it.  LRG_ASYNC_RT_HEAD_EVERY forces; unset: LRG_RT_HEAD_EVERY_AUTO above,
    //  unless LRG_ASYNC_RT_BB_EVERY asks for CUs with two branch teams by name -- the two never combine)
    A->rt_head_every = sw.rt_head_every != LRG_ENV_UNSET ? sw.rt_head_every : (sw.rt_bb_every != LRG_ENV_UNSET && sw.rt_bb_every > 0) ? 0 : LRG_RT_HEAD_EVERY_AUTO(n_slots);
    int worker_wgs = 0;                                     // workgroups of the worker kernel (wave-branch mode)
    int n_front = *n_front_io;
    int want = ab->branch_waves;
    if (want == 0 && n_slots >= LRG_REG_TILE_AUTO_MIN && n_slots <= LRG_REG_TILE_AUTO_MAX) want = 1;      // (register tiles where they win: include/lrg_hip.h)
    if (async_two_kernels_fit(*A, ab, weights, n_slots, wgs, cus) && want > 0) {
        // Both kernels' workgroups go round the 8 XCDs in turn, and inside an XCD round its 4 shader engines (8 CUs each) -- a workgroup whose engine has no CU
        // free WAITS for one instead of going elsewhere, and where a kernel's round starts depends on what was dispatched before.  So the grids are sized per
        // shader engine for ANY alignment of the two rounds: the front kernel's F = n_front + units workgroups put at most f = ceil(ceil(F / 8) / 4) on one
        // engine, the worker kernel may then have 8 - f per engine: W = 32 x (8 - f).  (Sized per XCD only -- 21 + 232 workgroups -- 7 of 10 launches gave up at the
        // start rendezvous with every workgroup arrived in the end: the last worker workgroups had waited for CUs that front workgroups held, tools/r06_wave_rendezvous.py;
        // tools/two_kernel_rendezvous.hip, profiles/r03_side_stream: "a kernel of another stream is only placed when EVERY shader engine has a CU to spare".)
        // Front workgroups are added while the engines they already claim have room and there are slots for them.
        const int engines = 32, per_engine = wgs / engines;
        const bool fronts_free = ab->front_workgroups <= 0 && !A->front.spec_k;      // (neither the caller nor speculation fixed them)
        if (fronts_free && sw.wave_fronts > 0) n_front = min(sw.wave_fronts, n_slots);
        int f = ((n_front + A->gemv_units + 7) / 8 + 3) / 4;
        if (fronts_free && sw.wave_fronts <= 0) n_front = max(n_front, min(n_slots, engines * f - A->gemv_units));
        const int F = n_front + A->gemv_units;
        f = ((F + 7) / 8 + 3) / 4;
        worker_wgs = engines * (per_engine - f);
        // (test hook: that many worker workgroups MORE than the shader engines hold -- a launch that can never be resident as a whole: its front workgroups
        //  give up at the start rendezvous with reason 6, the workgroups that start after that find the abort word and leave;
        //  tests/test_gpu_free_run.py::test_wave_branch_launch_that_cannot_be_resident_gives_up_cleanly)
        worker_wgs += max(0, sw.wave_extra_wgs);
        // (per evaluation ~7 tiles: PREFIX tasks ~7 x 10 us of one wavefront, POOL tasks ~28 x 9 us, four wavefronts to a CU; head tiles ~7 x 13-17 us of a team, two
        //  to a CU -- and the pooled blocks where there are no units: 62 % | 55 % of the worker CUs run branch tasks, a fifth of those the PREFIX tasks)
        int wave_wgs = sw.wave_wgs > 0 ? sw.wave_wgs : worker_wgs * (A->gemv_units ? 62 : 55) / 100;
        wave_wgs = max(8, min(wave_wgs / 4 * 4, worker_wgs - 8));
        int a_wgs = sw.wave_a_wgs > 0 ? sw.wave_a_wgs : (wave_wgs + 2) / 5;
        a_wgs = max(1, min(a_wgs, wave_wgs - 4));
        a_wgs += (wave_wgs - a_wgs) % 4;                     // (POOL CUs: a multiple of four -- the (side, half) kinds)
        size_t c3[2];
        if (want == 1) {
            // REGISTER TILES (LrgAsyncBuffers.branch_waves = 1): every worker workgroup alike -- team 0 the branch tiles (four wavefronts per tile, activations in
            // registers where that is free: lrg_team_branch_tile_reg), team 1 the pooled blocks and head tiles
            if (worker_wgs >= 24) A->reg_tiles = sw.rt_team_heads ? 2 : 1;      // (2: register branch tiles, team head tiles)
        } else if (worker_wgs >= 24 && lrg_packed_conv3_view(weights, n_slots, b->row_cap, c3) == 0) {
            A->wave_wgs = wave_wgs; A->wave_a_wgs = a_wgs;
            A->wave_waves = want > 0 ? min(want, 8) : 4;
            A->wave_split = sw.wave_split == 8 ? 8 : 4;
            A->h3[0] = static_cast<float *>(b->workspace) + c3[0]; A->h3[1] = static_cast<float *>(b->workspace) + c3[1];
        }
    }
    *n_front_io = n_front;
    return worker_wgs;
}

// (10a) Teams per worker CU: two -- the first runs branch tiles, the second head tiles (a tile beside another takes 1.2 x as long, but
// the head tiles wait inside for the pooled-product units, and at 68 slots the teams are what a step queues for: 1 / 2 / 3 teams
// 751 / 806 / 771 k instance-steps/s with 34 front workgroups, profiles/r03_units_sweep.log); one while the slots are few (nothing
// queues, a tile alone is faster: eight scenes 108 k against 97 k); three where hundreds of slots are in flight
// (the one-kernel launch's teams: a two-kernel launch has two, A.teams)
static int plan_teams(const LrgAsyncBuffers *ab, int n_slots, int gemv_units) {
    return ab->teams > 0 ? min(ab->teams, 4) : n_slots <= 24 ? 1 : n_slots <= 96 ? (gemv_units ? 2 : 1) : n_slots <= (gemv_units ? 128 : 200) ? 3 : 4;      // (112 slots: 2 / 3 teams 1.02 / 1.04 M; 96: 1.00 / 0.96 M)
}

// (10b) The fill-in teams of a launch with fill-in buffers (step 6), by the form of the launch.  Decides A->fill_wgs, wave_fill, fill_extra, fill_hybrid, and hands the
// fill-in back to the host (A->fill_list = nullptr, a->fill_in_launch = 0) where no team is left for it.
static void plan_fill_teams(const LrgAsyncBuffers *ab, const LrgAsyncSwitches &sw, int wgs, int n_front, int worker_wgs, int teams, LrgAsyncArgs *A, LrgFrontArgs *a) {
    if (A->fill_list && A->reg_tiles) {
        // both teams of a register-tile CU run tiles: the second team of the first fill_wgs of them serves the fill-in ring instead of ring 1 (LrgAsyncBuffers.fill_wgs).
        // Default 0: the host fills finished rooms in between launches -- 68 rooms in flight, 0 / 8 / 16 / 32 such workgroups: 931 / 892 / 918 / 920 k instance-steps/s
        // (profiles/r06_reg_tiles_sweep.txt): a head team less per CU costs more than the fill-ins between two launches
        const int want_fill = ab->fill_wgs > 0 ? ab->fill_wgs : 0;
        A->fill_wgs = min(want_fill, worker_wgs / 4);
        if (A->fill_wgs < 1) { A->fill_list = nullptr; a->fill_in_launch = 0; }
    } else if (A->fill_list && A->wave_wgs) {
        // the fill-in teams: wavefronts 4 .. 7 of wave-branch CUs (VALU work beside the MFMA-bound branch wavefronts of the same SIMDs), unless those run branch tasks too
        if (A->wave_waves <= 4) {
            A->wave_fill = 1;
            A->fill_wgs = ab->fill_wgs > 0 ? min(ab->fill_wgs, A->wave_wgs) : min(64, A->wave_wgs);
        } else {
            A->fill_list = nullptr; a->fill_in_launch = 0;    // (the host fills in between launches)
        }
    } else if (A->fill_list) {
        const int workers = wgs - n_front - A->gemv_units;
        // (16 / 32 / 64 / 103 such workgroups at 68 rooms in flight: 852 / 858 / 857 / 857 k instance-steps/s, 6: 804 k -- a big room's ~170 tasks queue for
        //  them; without the in-launch fill-in 852 k: profiles/r04_fill_in_launch_ab.txt)
        A->fill_wgs = ab->fill_wgs > 0 ? min(ab->fill_wgs, workers / 2) : min(64, workers / 3);      // (end of round 4, 2 176 rooms: 32 / 64 / 96 such workgroups 581 / 587 / 587 rooms/s at 68 slots, 839 / 856 / 844 at 272)
        if (A->fill_wgs < 1) { A->fill_list = nullptr; a->fill_in_launch = 0; }      // (too few workgroups: the host fills in)
        A->fill_extra = (A->fill_list && teams <= 3) ? 1 : 0;      // (a fourth team of 256 threads beside three tile teams; its LDS region is 16 KB)
        // four tile teams: the fill-in team is the CU's fourth tile team and serves ring 1 while no fill-in task waits (LRG_ASYNC_FILL_HYBRID=0: the fill-in ring only)
        A->fill_hybrid = (A->fill_list && teams == 4 && sw.fill_hybrid) ? 1 : 0;
    }
}

// (10b') Register-tile CUs by role (lrg_rt_role, lrg_async_plan.h): grants what plan_two_kernels left in A->rt_head_every, or takes it back.  One CU in N of an XCD's
// share of the worker grid (w / 8) runs head tiles on both teams, the others branch tiles on team 0 alone -- N is kept within 2 .. worker_wgs / 8, so that the grid
// has a CU of either role and neither ring is left without a team (a value below 2, or a grid of fewer than 16 workgroups: ignored).  Only where every CU is a
// plain register-tile CU: not with team head tiles (reg_tiles == 2), whose team 0 region is not a head team's, and not with fill-in teams, which take team 1 of
// the first CUs whatever their role.  Never beside two-branch-team CUs: a granted value makes rt_bb_every 0.  Decides A->rt_head_every, rt_bb_every.
static void plan_roles(int worker_wgs, LrgAsyncArgs *A) {
    int n = A->reg_tiles == 1 && !A->fill_wgs ? min(A->rt_head_every, worker_wgs / 8) : 0;
    if (n < 2) n = 0;
    A->rt_head_every = n;
    if (n) A->rt_bb_every = 0;
}

// (10c) Which team serves which ring, the small teams and the tasks per branch tile.  Decides A->ring0_halves, head_ring, small_teams, small_alt, poll_sleep,
// branch_parts -- and for a two-kernel launch overrides them with that form's (and takes back fill_extra).
static void plan_rings_and_parts(const LrgAsyncBuffers *ab, const LrgAsyncSwitches &sw, int n_slots, int teams, LrgAsyncArgs *A) {
    A->ring0_halves = sw.ring0_halves > 0 ? sw.ring0_halves : teams >= 3 ? 3 : 2;
    A->head_ring = (teams > 1 && (sw.ring0_halves >= 0 || teams == 4)) ? 1 : 0;      // (LRG_ASYNC_RING0_HALVES=-1: one ring)
    // four teams: 2 x (branch tile: 28 KB) + 2 x (head tile: 44.5 KB) = 145 KB of the CU's 160; the first two run branch tiles only
    A->small_teams = teams == 4 ? (sw.small_teams == 3 ? 3 : 2) : 0;
    A->small_alt = (teams == 4 && sw.small_teams == 23) ? 1 : 0;
    A->poll_sleep = ab->poll_sleep > 0 ? ab->poll_sleep : 1;
    // few slots, most teams idle: a branch tile as two tasks that share its pooled layer (tile 22.8 -> 18.4 us; eight 100 k-point scenes
    // 75.9 k -> 78.1 k instance-steps/s, four tasks 75.0 k; 68 rooms: 559 k -> 505 k, the teams are busy there: profiles/r03_parts_perf.log)
    A->branch_parts = ab->branch_parts > 0 ? (ab->branch_parts >= 4 ? 4 : ab->branch_parts >= 2 ? 2 : 1) : (n_slots <= 46 ? 2 : 1);      // (end of round 4, profiles/r04_teams_units_sweep.txt: 16 / 24 / 39 / 44 / 52 / 68 slots, 2 against 1 part: +8 / +6 / +2.3 / +1.5 / -2 / -17 %)
    if (A->wave_wgs) { A->branch_parts = A->wave_split; A->head_ring = 1; A->small_teams = 0; A->small_alt = 0; A->fill_extra = 0; }
    if (A->reg_tiles) {
        // (a register branch tile as two tasks where CUs idle: LrgAsyncBuffers.branch_parts >= 2, by default up to 24 slots)
        A->branch_parts = ab->branch_parts > 0 ? (ab->branch_parts >= 2 ? 2 : 1) : (n_slots <= 24 ? 2 : 1);
        A->head_ring = 1; A->small_teams = 0; A->small_alt = 0; A->fill_extra = 0;
    }      // (a branch tile = its four quarters; ring 1 for everything else)
}

// (11) The launch's limits in wall_clock64 ticks (100 MHz).  Decides A->max_steps, budget_ticks, abort_ticks, start_ticks.
static void plan_ticks(const LrgAsyncBuffers *ab, int max_steps, int budget_us, LrgAsyncArgs *A) {
    A->max_steps = max_steps;
    A->budget_ticks = budget_us > 0 ? (long long)budget_us * 100 : (1LL << 60);      // wall_clock64: 100 MHz
    A->abort_ticks = (budget_us > 0 ? (long long)budget_us * 100 : 0) + 400000000LL;  // ... + 4 s without an end: something is broken
    A->start_ticks = ab->start_wait_us > 0 ? (long long)ab->start_wait_us * 100 : (budget_us > 0 ? (long long)budget_us * 100 : 0) + LRG_ASYNC_START_TICKS;
}

// (12) Both kernels' dynamic LDS
static void plan_lds(const LrgAsyncArgs &A, int teams, bool two_kernels, size_t *lds, size_t *worker_lds) {
    static_assert(sizeof(LrgAsyncKArgs) <= 4096, "kernel arguments");
    // (+ the records of the prepared mask update, lrg_front.inl: with the pooled-product units on, less than the sixteen unit workgroups need anyway)
    const size_t front_lds = LRG_PREPARED_UPDATE ? LRG_ASYNC_FRONT_PREP_BYTES + LRG_PREP_SLOTS * sizeof(LrgPrepRecord)
                                                 : ((sizeof(LrgFrontShared) + 15) & ~(size_t)15) + sizeof(LrgAsyncFrontCtl);
    static_assert(LRG_ASYNC_FRONT_PREP_BYTES + LRG_PREP_SLOTS * sizeof(LrgPrepRecord) <= 160 * 1024, "a front workgroup with its records");
    // (small_alt: the odd workgroups have one small team more and one big team less -- the even ones' layout is the larger)
    const size_t team_lds = ((size_t)A.small_teams * LRG_ASYNC_SMALL_TEAM_FLOATS + (size_t)(teams - A.small_teams) * LRG_ASYNC_TEAM_FLOATS +
                             (size_t)A.fill_extra * LRG_ASYNC_FILL_TEAM_FLOATS) * sizeof(float);
    static_assert((3 * LRG_ASYNC_TEAM_FLOATS + LRG_ASYNC_FILL_TEAM_FLOATS) * sizeof(float) <= 160 * 1024, "three tile teams and a fill team per CU");
    static_assert((2 * LRG_ASYNC_SMALL_TEAM_FLOATS + 2 * LRG_ASYNC_TEAM_FLOATS) * sizeof(float) <= 160 * 1024, "four tile teams per CU");
    const size_t unit_lds = A.gemv_units ? (size_t)max((int)LRG_GEMV_UNIT_FLOATS(A.gemv.P), (int)LRG_GEMV_UNIT2_FLOATS(A.gemv.P)) * sizeof(float) + 16 : 0;
    *lds = (max(max(front_lds, two_kernels ? (size_t)0 : team_lds), unit_lds) + 15) & ~(size_t)15;
    // (wave-branch mode, the worker kernel: a wave-branch CU's kernels + its fill-in team | two tile teams)
    *worker_lds = (max(max((size_t)(LRG_WB_FLOATS + LRG_ASYNC_FILL_TEAM_FLOATS), (size_t)2 * LRG_ASYNC_TEAM_FLOATS),
                       (size_t)(LRG_RT_WEIGHT_FLOATS + LRG_RT_TEAM0_FLOATS + max((int)LRG_ASYNC_TEAM_FLOATS, (int)LRG_RT_TEAM1_FLOATS))) * sizeof(float) + 15) & ~(size_t)15;
    // (a HEAD2 CU, lrg_rt_role: its second head team's region lies over the branch kernels and team 0's exchange buffer, which it does not use -- worker_lds does not grow)
    static_assert(LRG_ASYNC_TEAM_FLOATS <= LRG_RT_WEIGHT_FLOATS + LRG_RT_TEAM0_FLOATS && LRG_RT_TEAM1_FLOATS <= LRG_RT_WEIGHT_FLOATS + LRG_RT_TEAM0_FLOATS,
                  "a head team's region in the place of the branch kernels and team 0's region");
    static_assert((LRG_WB_FLOATS + LRG_ASYNC_FILL_TEAM_FLOATS) * sizeof(float) <= 160 * 1024, "a wave-branch CU: the kernels of its (side, quarter) and a fill-in team");
}

// The launch's shape from the checked arguments (lrg_async_check), the device's CU count and the switches: no HIP call, no state
int lrg_async_plan(LrgSlot *slots, LrgRoom *rooms, int n_slots, int max_points, const LrgGrowParams *params, const LrgWeights *weights,
                   const LrgPackedBuffers *b, const LrgAsyncBuffers *ab, int max_steps, int budget_us, int cus, const LrgAsyncSwitches &sw,
                   LrgAsyncPlan *plan) {
    LrgAsyncKArgs &K = plan->K;
    K.slots = slots; K.rooms = rooms; K.prm = *params;
    LrgAsyncArgs &A = K.A;
    LrgFrontArgs &a = A.front;
    const int row_stride = async_row_stride(params);
    int rc, wgs, n_front;
    bool tails_on;
    if ((rc = plan_problems(weights, b, n_slots, A.prob, &A.gemv))) return rc;
    if ((rc = plan_front_args(params, weights, b, ab, n_slots, row_stride, &a, A.prob))) return rc;
    if ((rc = plan_front_workgroups(ab, n_slots, cus, &wgs, &tails_on, &n_front))) return rc;
    if ((rc = plan_speculation(ab, n_slots, wgs, &a, &n_front))) return rc;
    plan_units(ab, weights, sw, A.gemv, n_slots, cus, wgs, tails_on, n_front, &A);
    if ((rc = plan_fill_buffers(ab, params, max_points, &A, &a))) return rc;
    if ((rc = plan_tail_tiles(ab, b, sw, n_slots, row_stride, a.rows16, A.gemv_units, &A, &a, &plan->tail_ctl_bytes))) return rc;
    if ((rc = plan_pool_rows(ab, n_slots, row_stride, A.gemv_units, A.gemv.P, &A, &a))) return rc;
    const int worker_wgs = plan_two_kernels(ab, weights, b, sw, n_slots, wgs, cus, &A, &n_front);
    const int teams = plan_teams(ab, n_slots, A.gemv_units);
    const bool two_kernels = A.wave_wgs || A.reg_tiles;
    A.queue = ab->queue; A.sync = ab->sync; A.big = b->slot_big; A.room_queue = ab->room_queue; A.work = reinterpret_cast<unsigned long long *>(ab->work); A.dbg = reinterpret_cast<unsigned long long *>(ab->debug_ticks);
    A.qmask = (int)async_ring_entries(n_slots) - 1;
    A.gmask = (int)async_unit_ring_entries(n_slots) - 1;
    A.n_slots = n_slots; A.n_front = n_front; A.teams = two_kernels ? 2 : teams;
    A.worker_base = n_front + A.gemv_units; A.total_wgs = two_kernels ? n_front + A.gemv_units + worker_wgs : wgs;
    plan_fill_teams(ab, sw, wgs, n_front, worker_wgs, teams, &A, &a);
    plan_roles(worker_wgs, &A);
    plan_rings_and_parts(ab, sw, n_slots, teams, &A);
    plan_ticks(ab, max_steps, budget_us, &A);
    plan_lds(A, teams, two_kernels, &plan->lds, &plan->worker_lds);
    plan->two_kernels = two_kernels;
    plan->front_wgs = two_kernels ? n_front + A.gemv_units : wgs;
    plan->worker_wgs = worker_wgs;
    plan->need_cus = two_kernels ? cus : wgs;                // (the two grids are sized for the whole chip)
    return 0;
}

// The launch as planned: the memsets, the residency checks and the one or two kernels
static int async_launch(const LrgAsyncPlan &plan, int cus, hipStream_t st) {
    const LrgAsyncKArgs &K = plan.K;
    if (plan.tail_ctl_bytes) LRG_HIP_CHECK(hipMemsetAsync(K.A.tail, 0, plan.tail_ctl_bytes, st));
    LRG_HIP_CHECK(hipMemsetAsync(K.A.queue, 0, lrg_grow_async_queue_bytes(K.A.n_slots), st));
    LRG_HIP_CHECK(hipMemsetAsync(K.A.sync, 0, (size_t)K.A.n_slots * LRG_ASYNC_SYNC_WORDS * sizeof(int32_t), st));
    static bool attr_done[LRG_MAX_DEVICES] = {};
    const int dev = lrg_current_device();
    if (!attr_done[dev]) {
        LRG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(lrg_grow_async_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        LRG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(lrg_grow_async_worker_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_done[dev] = true;
    }
    // Residency: front workgroups, units and tile teams wait for each other, so the launch is only correct when ALL its workgroups run at
    // once -- one per CU.  Checked here instead of found out by a spin bound seconds later: the kernel as compiled must fit a CU with this
    // much LDS, and the stream must be allowed at least `wgs` CUs (a CU-masked stream, hipExtStreamCreateWithCUMask, is allowed fewer).
    // What cannot be seen from here (another process or stream holding CUs) is caught by the launch's own start rendezvous within
    // LRG_ASYNC_START_TICKS (lrg_async.inl: abort reason 6), not by the hand-overs' multi-second bounds.
    {
        int per_cu = 0;
        LRG_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(lrg_grow_async_kernel), LRG_FRONT_THREADS, plan.lds));
        if (per_cu < 1) return LRG_ERESIDENCY;
        if (plan.two_kernels) {
            LRG_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void *>(lrg_grow_async_worker_kernel), LRG_WORKER_THREADS, plan.worker_lds));
            if (per_cu < 1) return LRG_ERESIDENCY;
        }
        uint32_t cumask[32] = {};
        const uint32_t words = (uint32_t)min(32, (cus + 31) / 32);
        if (hipExtStreamGetCUMask(st, words, cumask) == hipSuccess) {
            int visible = 0;
            for (uint32_t i = 0; i < words; ++i) visible += __builtin_popcount(cumask[i]);
            if (visible > 0 && visible < plan.need_cus) return LRG_ERESIDENCY;      // (no bit set: no mask reported)
        } else {
            (void)hipGetLastError();
        }
    }
    if (plan.two_kernels) {
        // Two kernels, resident together: the worker kernel on the side stream between two events of the caller's stream (it starts after everything the caller
        // enqueued before this call -- the memsets above included -- and the caller's stream goes on only when it has left), the front kernel on the caller's stream.
        LrgSideStream *side = lrg_side_stream();
        if (!side) return LRG_ERESIDENCY;
        LrgAsyncKArgs KW = K;
        KW.A.worker_base = K.A.wave_wgs;                     // (the tile teams' workgroups are numbered from the first one behind the wave-branch CUs)
        const unsigned ev = side->next++ % LRG_SIDE_EVENTS;
        LRG_HIP_CHECK(hipEventRecord(side->start[ev], st));
        LRG_HIP_CHECK(hipStreamWaitEvent(side->stream, side->start[ev], 0));
        hipLaunchKernelGGL(lrg_grow_async_worker_kernel, dim3(plan.worker_wgs), dim3(LRG_WORKER_THREADS), plan.worker_lds, side->stream, KW);
        LRG_LAUNCH_CHECK();
        LRG_HIP_CHECK(hipEventRecord(side->done[ev], side->stream));
        hipLaunchKernelGGL(lrg_grow_async_kernel, dim3(plan.front_wgs), dim3(LRG_FRONT_THREADS), plan.lds, st, K);
        LRG_LAUNCH_CHECK();
        LRG_HIP_CHECK(hipStreamWaitEvent(st, side->done[ev], 0));
        return 0;
    }
    hipLaunchKernelGGL(lrg_grow_async_kernel, dim3(plan.front_wgs), dim3(LRG_FRONT_THREADS), plan.lds, st, K);
    LRG_LAUNCH_CHECK();
    return 0;
}

// what the process's last lrg_grow_async planned (lrg_async_last_plan, lrg_async_plan.h; for tests and tools: callers that launch from several threads see any one of them)
static int32_t async_last_plan[LRG_ASYNC_LAST_PLAN_WORDS] = {};

int lrg_grow_async(LrgSlot *slots, LrgRoom *rooms, int n_slots, int max_points, const LrgGrowParams *params, const LrgWeights *weights,
                   const LrgPackedBuffers *b, const LrgAsyncBuffers *ab, int max_steps, int budget_us, void *stream) {
    int rc = lrg_async_check(slots, rooms, n_slots, max_points, params, weights, b, ab, max_steps, budget_us);
    if (rc) return rc;
    hipDeviceProp_t prop;
    LRG_HIP_CHECK(hipGetDeviceProperties(&prop, lrg_current_device()));
    LrgAsyncPlan plan;
    if ((rc = lrg_async_plan(slots, rooms, n_slots, max_points, params, weights, b, ab, max_steps, budget_us, prop.multiProcessorCount, lrg_async_switches(), &plan)))
        return rc;
    {
        const LrgAsyncArgs &A = plan.K.A;
        const int32_t v[LRG_ASYNC_LAST_PLAN_WORDS] = {1, plan.two_kernels ? 1 : 0, plan.front_wgs, plan.worker_wgs, A.n_front, A.gemv_units, A.unit_pairs, A.unit_regs, A.reg_tiles, A.teams,
                                                      A.pool_rows ? 1 : 0, A.n_slots};
        for (int i = 0; i < LRG_ASYNC_LAST_PLAN_WORDS; ++i) async_last_plan[i] = v[i];
    }
    return async_launch(plan, prop.multiProcessorCount, (hipStream_t)stream);
}

int lrg_async_last_plan(int32_t *out, int n) {
    if (!out || n < 0) return LRG_EINVAL;
    for (int i = 0; i < n && i < LRG_ASYNC_LAST_PLAN_WORDS; ++i) out[i] = async_last_plan[i];
    return min(n, LRG_ASYNC_LAST_PLAN_WORDS);
}
