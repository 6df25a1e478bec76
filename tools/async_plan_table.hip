// The launch plans of lrg_grow_async (csrc/lrg_async_plan.inl: lrg_async_check, lrg_async_plan) over a fixed sweep of cases, one line per case:
//
//     label|return code|the deciding scalars, in the order of the '#' line (0*k: k zeros)|CRC-32 of the canonical text of the whole plan        (a refusal: label|return code)
//
// and, behind them, one 'Q' line per slot count: where the rings the plans address end in the queue, and the words lrg_grow_async_queue_bytes gives it.
// --full prints the canonical text itself behind every line.  tests/test_async_plan.py compares the output with tests/golden/async_plan_table.txt, so that
// a change to a decision of the plan shows as the launches it moves.
// --roles prints another table instead: the register-tile CUs by role over the same sweep (roles_rows below; tests/test_async_roles.py).
// --unit-regs prints a third: the form of the pooled-product units over the same sweep (unit_regs_rows below; tests/test_async_unit_regs.py).
//
// No kernel and no HIP call: the plan is a function of its arguments, the CU count and the switches.  Every address is made up (a region number in the bits
// from 40 up, an offset below) and none is dereferenced; the text names pointers by region and offset, never by value, and never prints a struct's raw bytes.
// The switches are passed in the struct (their defaults: what lrg_async_switches reads from an empty environment).
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off tools/async_plan_table.hip -o tools/build/async_plan_table
//              -L learn_region_grow_amd -l:liblrg_hip.so -Wl,-rpath,<that directory>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <vector>
#include <algorithm>
#include "../learn_region_grow_amd/csrc/lrg_async_plan.h"

// ---- made-up addresses ----
enum Region { R_NULL, R_SLOTS, R_ROOMS, R_CENTER, R_SAMPLE_IN, R_SAMPLE_NB, R_X_IN, R_X_NB, R_ROW_SLOT_IN, R_ROW_SLOT_NB, R_UPD_IN, R_UPD_NB, R_RMV_LOGITS,
              R_ADD_LOGITS, R_SLOT_ROWS, R_COUNTERS, R_WORKSPACE, R_STATS, R_SLOT_BIG, R_QUEUE, R_SYNC, R_ROOM_QUEUE, R_WORK, R_FILL_LIST, R_FILL_BEST, R_FILL_SYNC,
              R_FILL_LABEL, R_FILL_OUT, R_POOL_ROWS, R_DEBUG, R_TAIL_CTL, R_PACKED, R_INLIER_W, R_INLIER_B, R_NEIGHBOR_W, R_NEIGHBOR_B, R_ADD_W, R_ADD_B, R_RMV_W,
              R_RMV_B, R_COUNT };
static const char *const REGION_NAME[R_COUNT] = {
    "null", "slots", "rooms", "center", "sample_in", "sample_nb", "x_in", "x_nb", "row_slot_in", "row_slot_nb", "upd_in", "upd_nb", "rmv_logits", "add_logits",
    "slot_rows", "counters", "workspace", "stats", "slot_big", "queue", "sync", "room_queue", "work", "fill_list", "fill_best", "fill_sync", "fill_label",
    "fill_out", "pool_rows", "debug", "tail_ctl", "packed", "inlier_w", "inlier_b", "neighbor_w", "neighbor_b", "add_w", "add_b", "rmv_w", "rmv_b"};
template <typename T = void> static T *at(Region r, size_t off = 0) { return reinterpret_cast<T *>(((uintptr_t)r << 40) + off); }
static std::string ptr_text(const void *p) {
    if (!p) return "null";
    const uintptr_t v = (uintptr_t)p, r = v >> 40;
    char buf[64];
    if (r == 0 || r >= R_COUNT) snprintf(buf, sizeof(buf), "?%llx", (unsigned long long)v);      // (not one of ours: a field the plan left unset)
    else snprintf(buf, sizeof(buf), "%s+%llu", REGION_NAME[r], (unsigned long long)(v & (((uintptr_t)1 << 40) - 1)));
    return buf;
}

static unsigned crc32(const std::string &s) {
    unsigned c = 0xFFFFFFFFu;
    for (unsigned char ch : s) {
        c ^= ch;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
    }
    return ~c;
}

// ---- a case: the arguments of one lrg_grow_async call ----
enum Net { PAPER, LITE2, HEADS128, WIDE1, HEADS256_64 };
struct Setup {
    int n_slots, cus, max_points, max_steps, budget_us;
    LrgSlot *slots;
    LrgRoom *rooms;
    LrgGrowParams prm;
    LrgWeights w;
    LrgPackedBuffers b;
    LrgAsyncBuffers ab;
    LrgAsyncSwitches sw;
    int net;
};

static LrgAsyncSwitches default_switches;

static int row_stride_of(const Setup &S) { return ((S.prm.n_inlier > S.prm.n_neighbor ? S.prm.n_inlier : S.prm.n_neighbor) + 31) / 32 * 32; }
// (the row arrays and the workspace follow row_cap)
static void set_row_cap(Setup &S, int row_cap) {
    S.b.row_cap = row_cap;
    S.b.workspace_bytes = lrg_forward_packed_workspace_bytes(&S.w, S.n_slots, row_cap);
}

static Setup make(int n_slots, int cus, int net, int features, int n_inlier, int n_neighbor) {
    Setup S;
    memset(&S, 0, sizeof(S));
    S.n_slots = n_slots; S.cus = cus; S.net = net;
    S.max_points = 65536; S.max_steps = 64; S.budget_us = 500;
    S.slots = at<LrgSlot>(R_SLOTS); S.rooms = at<LrgRoom>(R_ROOMS);
    S.prm.resolution = 0.1f; S.prm.feature_size = features; S.prm.n_inlier = n_inlier; S.prm.n_neighbor = n_neighbor;
    S.prm.cluster_threshold = 10; S.prm.restarts = 1; S.prm.group_size = 1; S.prm.max_region_steps = 0; S.prm.rng_seed = 1; S.prm.policy = 0; S.prm.scoring = 0;
    static const int conv[5][5] = {{64, 64, 64, 128, 512}, {64, 64, 256, 0, 0}, {64, 64, 64, 128, 512}, {64, 128, 64, 128, 512}, {64, 64, 64, 128, 512}};
    static const int head[5][3] = {{256, 128, 2}, {64, 64, 2}, {128, 64, 2}, {256, 128, 2}, {256, 64, 2}};      // (the last: the paper's but for the second width)
    LrgWeights &w = S.w;
    w.feature_size = features; w.n_conv = net == LITE2 ? 3 : 5; w.n_head = 3;
    for (int i = 0; i < w.n_conv; ++i) {
        w.conv_ch[i] = conv[net][i];
        w.inlier_w[i] = at<float>(R_INLIER_W, (size_t)i << 24); w.inlier_b[i] = at<float>(R_INLIER_B, (size_t)i << 24);
        w.neighbor_w[i] = at<float>(R_NEIGHBOR_W, (size_t)i << 24); w.neighbor_b[i] = at<float>(R_NEIGHBOR_B, (size_t)i << 24);
    }
    for (int i = 0; i < w.n_head; ++i) {
        w.head_ch[i] = head[net][i];
        w.add_w[i] = at<float>(R_ADD_W, (size_t)i << 24); w.add_b[i] = at<float>(R_ADD_B, (size_t)i << 24);
        w.rmv_w[i] = at<float>(R_RMV_W, (size_t)i << 24); w.rmv_b[i] = at<float>(R_RMV_B, (size_t)i << 24);
    }
    w.packed = at(R_PACKED);
    LrgPackedBuffers &b = S.b;
    b.center = at<float>(R_CENTER); b.sample_in = at<int32_t>(R_SAMPLE_IN); b.sample_nb = at<int32_t>(R_SAMPLE_NB);
    b.x_in = at<float>(R_X_IN); b.x_nb = at<float>(R_X_NB); b.row_slot_in = at<int32_t>(R_ROW_SLOT_IN); b.row_slot_nb = at<int32_t>(R_ROW_SLOT_NB);
    b.upd_in = at<float>(R_UPD_IN); b.upd_nb = at<float>(R_UPD_NB); b.rmv_logits = at<float>(R_RMV_LOGITS); b.add_logits = at<float>(R_ADD_LOGITS);
    b.slot_rows = at<int32_t>(R_SLOT_ROWS); b.counters = at<int32_t>(R_COUNTERS); b.workspace = at(R_WORKSPACE); b.stats = at<int64_t>(R_STATS);
    b.rooms_have_pvox = 1; b.slot_big = at<int32_t>(R_SLOT_BIG);
    set_row_cap(S, n_slots * row_stride_of(S) + 4096 + 32);      // (room for 4096 shared tail rows)
    LrgAsyncBuffers &ab = S.ab;
    ab.queue = at<int32_t>(R_QUEUE); ab.queue_bytes = lrg_grow_async_queue_bytes(n_slots); ab.sync = at<int32_t>(R_SYNC);
    ab.room_queue = at<int32_t>(R_ROOM_QUEUE); ab.work = at<uint64_t>(R_WORK); ab.rows16 = 1;
    S.sw = default_switches;
    return S;
}
static Setup paper(int n_slots, int cus = 256) { return make(n_slots, cus, PAPER, 13, 512, 512); }

static void grant_tails(Setup &S, int rows = 4096) { S.ab.tail_ctl = at<int32_t>(R_TAIL_CTL); S.ab.tail_rows = rows; }
static void grant_pool_rows(Setup &S) { S.ab.pool_rows = at<float>(R_POOL_ROWS); S.ab.pool_rows_bytes = lrg_grow_async_pool_rows_bytes(&S.w, S.n_slots); }
static void grant_fill(Setup &S, int fill_wgs) {
    S.ab.fill_list = at<int32_t>(R_FILL_LIST); S.ab.fill_best = at<uint64_t>(R_FILL_BEST); S.ab.fill_sync = at<int32_t>(R_FILL_SYNC);
    S.ab.fill_label_base = at<int32_t>(R_FILL_LABEL); S.ab.fill_out_base = at<int32_t>(R_FILL_OUT); S.ab.fill_rooms = 100; S.ab.fill_wgs = fill_wgs;
}

// ---- the canonical text of a plan: every field of LrgAsyncPlan, LrgAsyncKArgs, LrgAsyncArgs and LrgFrontArgs, the problems and the pooled product ----
struct Text {
    std::string s;
    void num(const char *k, long long v) { char b[96]; snprintf(b, sizeof(b), "%s=%lld\n", k, v); s += b; }
    void ptr(const char *k, const void *p) { s += k; s += '='; s += ptr_text(p); s += '\n'; }
};
#define N(x) T.num(#x, (long long)(x))
#define P(x) T.ptr(#x, (const void *)(x))
static void problem_text(Text &T, int i, const LrgFusedProb &p) {
    T.num("prob", i);
    P(p.x); P(p.pool); P(p.fw); P(p.fb); P(p.fout); P(p.valid); P(p.tile_count); P(p.tile_list); P(p.zero_pool); P(p.pool_rows); N(p.pool_rows_stride); P(p.nrows);
    P(p.row_inst); P(p.center); N(p.rows); N(p.ldx); N(p.Kin); N(p.rows_per_inst); N(p.pool_stride); N(p.nlayers); N(p.zero_count);
    for (int l = 0; l < p.nlayers && l < LRG_FUSED_MAXL; ++l) {
        const LrgFusedLayer &L = p.L[l];
        T.num("layer", l);
        P(L.w); P(L.bias); P(L.gout); N(L.K); N(L.N); N(L.ng); N(L.flags);
    }
}
static std::string plan_text(const LrgAsyncPlan &plan) {
    Text T;
    N(plan.two_kernels); N(plan.front_wgs); N(plan.worker_wgs); N(plan.lds); N(plan.worker_lds); N(plan.need_cus); N(plan.tail_ctl_bytes);
    const LrgAsyncKArgs &K = plan.K;
    P(K.slots); P(K.rooms);
    { char b[64]; snprintf(b, sizeof(b), "K.prm.resolution=%.9g\n", (double)K.prm.resolution); T.s += b; }
    N(K.prm.feature_size); N(K.prm.n_inlier); N(K.prm.n_neighbor); N(K.prm.cluster_threshold); N(K.prm.restarts); N(K.prm.group_size); N(K.prm.max_region_steps);
    N(K.prm.rng_seed); N(K.prm.policy); N(K.prm.scoring);
    const LrgAsyncArgs &A = K.A;
    for (int i = 0; i < 4; ++i) problem_text(T, i, A.prob[i]);
    const LrgGemvArgs &g = A.gemv;
    P(g.pooled); P(g.w[0]); P(g.w[1]); P(g.bias[0]); P(g.bias[1]); P(g.hb[0]); P(g.hb[1]); N(g.ldw); N(g.B); N(g.P); N(g.C); P(g.cnt_src); P(g.cnt_dst);
    const LrgFrontArgs &a = A.front;
    P(a.center); P(a.sample_in); P(a.sample_nb); P(a.x_in); P(a.x_nb); P(a.row_slot_in); P(a.row_slot_nb); P(a.upd_in); P(a.upd_nb); P(a.rmv_logits); P(a.add_logits);
    P(a.slot_rows); P(a.counters); P(a.pooled); N(a.pooled_stride); P(a.stats); P(a.phase_ticks); N(a.own_medians); P(a.phase_dbg); N(a.row_stride); N(a.rows16);
    N(a.fill_in_launch); P(a.tail_cur); P(a.tail_base); N(a.tail_rows); N(a.tail_row0); P(a.spec_stats); N(a.spec_k);
    P(A.queue); P(A.sync); P(A.big); P(A.room_queue); N(A.qmask); N(A.gmask); N(A.gemv_batch); N(A.gemv_batch_ticks); N(A.gemv_units); N(A.n_slots); N(A.n_front);
    N(A.teams); N(A.head_ring); N(A.ring0_halves); P(A.fill_list); P(A.fill_best); P(A.fill_sync); P(A.fill_label_base); P(A.fill_out_base); N(A.fill_wgs);
    N(A.small_teams); N(A.small_alt); N(A.fill_extra); N(A.fill_hybrid); P(A.tail); N(A.tail_tiles); N(A.tail_heads); N(A.tail_ticks); P(A.pool_rows);
    N(A.pool_rows_stride); N(A.poll_sleep); N(A.branch_parts); N(A.wave_wgs); N(A.wave_a_wgs); N(A.wave_waves); N(A.wave_split); N(A.wave_fill); N(A.wmask);
    P(A.h3[0]); P(A.h3[1]); N(A.rt_bb_every); N(A.unit_pairs); N(A.reg_tiles); N(A.worker_base); N(A.total_wgs); N(A.max_steps); N(A.start_ticks);
    N(A.budget_ticks); N(A.abort_ticks); P(A.work); P(A.dbg);
    return T.s;
}
#undef N
#undef P

// the deciding scalars of a line, in this order (the three rings by the logarithm of their entries: they are powers of two, which log2_entries checks)
static long long log2_entries(int mask) {
    int k = 0;
    while (k < 31 && (1LL << k) != (long long)mask + 1) ++k;
    if (k == 31) { fprintf(stderr, "async_plan_table: a ring of %lld entries\n", (long long)mask + 1); exit(2); }
    return k;
}
static const char *const COLUMNS =
    "# label|rc|front_wgs worker_wgs lds worker_lds need_cus n_front gemv_units unit_pairs gemv_batch teams reg_tiles wave_wgs wave_a_wgs wave_waves wave_split "
    "wave_fill log2(wmask+1) branch_parts log2(qmask+1) log2(gmask+1) ring0_halves head_ring small_teams small_alt fill_wgs fill_extra fill_hybrid fill_in_launch tail_tiles tail_heads "
    "tail_ticks pool_rows_stride rt_bb_every spec_k budget_ticks abort_ticks start_ticks|crc32";
static std::string scalars_text(const LrgAsyncPlan &p) {
    const LrgAsyncArgs &A = p.K.A;
    const long long v[] = {p.front_wgs, p.worker_wgs, (long long)p.lds, (long long)p.worker_lds, p.need_cus, A.n_front, A.gemv_units, A.unit_pairs, A.gemv_batch, A.teams,
                           A.reg_tiles, A.wave_wgs, A.wave_a_wgs, A.wave_waves, A.wave_split, A.wave_fill, log2_entries(A.wmask), A.branch_parts, log2_entries(A.qmask), log2_entries(A.gmask), A.ring0_halves,
                           A.head_ring, A.small_teams, A.small_alt, A.fill_wgs, A.fill_extra, A.fill_hybrid, A.front.fill_in_launch, A.tail_tiles, A.tail_heads,
                           A.tail_ticks, A.pool_rows_stride, A.rt_bb_every, A.front.spec_k, A.budget_ticks, A.abort_ticks, A.start_ticks};
    std::string s;
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n;) {
        int zeros = 0;
        while (i + zeros < n && v[i + zeros] == 0) ++zeros;
        s += s.empty() ? "" : " ";
        if (zeros >= 3) { s += "0*" + std::to_string(zeros); i += zeros; }      // (a run of zeros, to keep the table small)
        else s += std::to_string(v[i++]);
    }
    return s;
}

// ---- the run ----
static bool full = false;
static int rows = 0, refused = 0;
static std::set<int> check_codes, plan_codes;
static std::set<std::string> labels;
static std::map<int, long long> ring_end;      // by slot count: the end of the last wave ring over the granted plans, in words of the queue
static int lite2_rows = 0, lite2_pairs = 0, heads_rows = 0, heads_reg = 0, lds_over = 0;

// ---- --roles: the register-tile CUs by role (lrg_rt_role, csrc/lrg_async_plan.h) ----
// For every case of the sweep, the plan with the switch rt_head_every unset, 0, 2, 3, 4 and 64.  A granted register-tile row prints one line per value:
//     label|value|rt_head_every rt_bb_every|CUs MIXED BRANCH2 BRANCH1 HEAD2|teams on ring 0, on ring 1, on the fill-in ring|the fewest ring-0 / ring-1 teams on 8 consecutive workgroups
// every other granted row one line, label|-|the six plans' rt_head_every (all 0: no roles without register tiles).  The teams are counted with the kernel's
// own functions, lrg_rt_role and lrg_rt_team_ring, over the worker grid.  Exit code 1: a granted row with a ring that no team serves, with rt_head_every beside
// rt_bb_every, or with roles and no register tiles.  tests/test_async_roles.py compares the output with tests/golden/async_roles_table.txt.
static bool roles = false;
static int roles_bad = 0;
static void roles_rows(const std::string &label, const Setup &S0) {
    static const char *const names[6] = {"unset", "0", "2", "3", "4", "64"};
    const int values[6] = {default_switches.rt_head_every, 0, 2, 3, 4, 64};
    static LrgAsyncPlan plan;
    std::string plain = label + "|-|";
    bool reg = false;
    for (int i = 0; i < 6; ++i) {
        Setup S = S0;
        S.sw.rt_head_every = values[i];
        memset(static_cast<void *>(&plan), 0xA5, sizeof(plan));
        if (lrg_async_check(S.slots, S.rooms, S.n_slots, S.max_points, &S.prm, &S.w, &S.b, &S.ab, S.max_steps, S.budget_us) ||
            lrg_async_plan(S.slots, S.rooms, S.n_slots, S.max_points, &S.prm, &S.w, &S.b, &S.ab, S.max_steps, S.budget_us, S.cus, S.sw, &plan))
            return;                                  // (a refusal: no row)
        const LrgAsyncArgs &A = plan.K.A;
        if (A.rt_head_every && A.rt_bb_every) { fprintf(stderr, "async_plan_table: %s/%s: rt_head_every %d beside rt_bb_every %d\n", label.c_str(), names[i], A.rt_head_every, A.rt_bb_every); roles_bad = 1; }
        if (!A.reg_tiles) {
            if (A.rt_head_every) { fprintf(stderr, "async_plan_table: %s/%s: roles without register tiles\n", label.c_str(), names[i]); roles_bad = 1; }
            plain += (i ? " " : "") + std::to_string(A.rt_head_every);
            continue;
        }
        reg = true;
        const int W = plan.worker_wgs - A.wave_wgs;  // (the register-tile CUs: the worker grid)
        int cus[4] = {0, 0, 0, 0}, teams[3] = {0, 0, 0}, least[2] = {1 << 30, 1 << 30};
        std::vector<int> on0(W + 1, 0), on1(W + 1, 0);      // prefix sums of the teams per workgroup on ring 0 / ring 1
        for (int w = 0; w < W; ++w) {
            const int role = lrg_rt_role(w, A.rt_bb_every, A.rt_head_every);
            ++cus[role];
            int r0 = 0, r1 = 0;
            for (int t = 0; t < 2; ++t) {
                const int ring = (t && A.fill_list && w < A.fill_wgs) ? 2 : lrg_rt_team_ring(role, t);      // (the kernel's order: a fill-in team first)
                if (ring >= 0) ++teams[ring];
                r0 += ring == 0; r1 += ring == 1;
            }
            on0[w + 1] = on0[w] + r0; on1[w + 1] = on1[w] + r1;
        }
        for (int w = 0; w + 8 <= W; ++w) {
            least[0] = std::min(least[0], on0[w + 8] - on0[w]);
            least[1] = std::min(least[1], on1[w + 8] - on1[w]);
        }
        if (!teams[0] || !teams[1]) { fprintf(stderr, "async_plan_table: %s/%s: %d teams on ring 0, %d on ring 1\n", label.c_str(), names[i], teams[0], teams[1]); roles_bad = 1; }
        printf("%s|%s|%d %d|%d %d %d %d|%d %d %d|%d %d\n", label.c_str(), names[i], A.rt_head_every, A.rt_bb_every, cus[LRG_RT_MIXED], cus[LRG_RT_BRANCH2], cus[LRG_RT_BRANCH1],
               cus[LRG_RT_HEAD2], teams[0], teams[1], teams[2], least[0], least[1]);
    }
    if (!reg) printf("%s\n", plain.c_str());
}

// ---- --unit-regs: the form of the pooled-product units (LrgAsyncArgs.unit_regs, the switch LRG_ASYNC_UNIT_REGS) ----
// For every granted case of the sweep one line, the plan with the switch unset, 0 and 1:
//     label|gemv_units unit_pairs|unit_regs with the switch unset, 0, 1|lds with the switch unset, 0, 1
// Exit code 1: the register form without units, or for other heads than the paper's (1024 pooled features, 256 columns), or forced off and still on, or a plan
// whose units, half-teams or LDS move with the switch.
static bool unit_regs = false;
static int unit_regs_bad = 0;
static void unit_regs_rows(const std::string &label, const Setup &S0) {
    static LrgAsyncPlan plan[3];
    const int values[3] = {default_switches.unit_regs, 0, 1};
    if (lrg_async_check(S0.slots, S0.rooms, S0.n_slots, S0.max_points, &S0.prm, &S0.w, &S0.b, &S0.ab, S0.max_steps, S0.budget_us)) return;
    for (int i = 0; i < 3; ++i) {
        Setup S = S0;
        S.sw.unit_regs = values[i];
        memset(static_cast<void *>(&plan[i]), 0xA5, sizeof(plan[i]));
        if (lrg_async_plan(S.slots, S.rooms, S.n_slots, S.max_points, &S.prm, &S.w, &S.b, &S.ab, S.max_steps, S.budget_us, S.cus, S.sw, &plan[i])) return;
    }
    const LrgAsyncArgs &A = plan[0].K.A;
    bool bad = false;
    for (int i = 0; i < 3; ++i) {
        const LrgAsyncArgs &B = plan[i].K.A;
        const bool papers_heads = B.gemv.P == 1024 && B.gemv.C == 256;
        if (B.unit_regs != 0 && B.unit_regs != 1) bad = true;
        if (B.unit_regs && (!B.gemv_units || !papers_heads)) bad = true;
        if (B.gemv_units != A.gemv_units || B.unit_pairs != A.unit_pairs || plan[i].lds != plan[0].lds || plan[i].front_wgs != plan[0].front_wgs) bad = true;
    }
    if (plan[1].K.A.unit_regs) bad = true;
    if (plan[2].K.A.unit_regs != ((A.gemv_units && A.gemv.P == 1024 && A.gemv.C == 256) ? 1 : 0)) bad = true;
    if (bad) { fprintf(stderr, "async_plan_table: %s: the units' register form where it must not be, or a plan that moves with its switch\n", label.c_str()); unit_regs_bad = 1; }
    printf("%s|%d %d|%d %d %d|%lld %lld %lld\n", label.c_str(), A.gemv_units, A.unit_pairs, A.unit_regs, plan[1].K.A.unit_regs, plan[2].K.A.unit_regs,
           (long long)plan[0].lds, (long long)plan[1].lds, (long long)plan[2].lds);
}

static void run(const std::string &label, const Setup &S) {
    if (!labels.insert(label).second) { fprintf(stderr, "async_plan_table: label used twice: %s\n", label.c_str()); exit(2); }
    if (roles) { roles_rows(label, S); return; }
    if (unit_regs) { unit_regs_rows(label, S); return; }
    static LrgAsyncPlan plan;
    memset(static_cast<void *>(&plan), 0xA5, sizeof(plan));      // (a field that the plan leaves unset shows as that pattern, not as what the last case left)
    int rc = lrg_async_check(S.slots, S.rooms, S.n_slots, S.max_points, &S.prm, &S.w, &S.b, &S.ab, S.max_steps, S.budget_us);
    if (rc) check_codes.insert(rc);
    else if ((rc = lrg_async_plan(S.slots, S.rooms, S.n_slots, S.max_points, &S.prm, &S.w, &S.b, &S.ab, S.max_steps, S.budget_us, S.cus, S.sw, &plan)))
        plan_codes.insert(rc);
    ++rows;
    std::string text = "rc=" + std::to_string(rc) + "\n";
    if (rc) {
        ++refused;
        printf("%s|%d\n", label.c_str(), rc);
    } else {
        text += plan_text(plan);
        printf("%s|0|%s|%08x\n", label.c_str(), scalars_text(plan).c_str(), crc32(text));
        const LrgAsyncArgs &A = plan.K.A;
        const long long end = LRG_AQ_WAVE_RING(A, 8);
        if (end > ring_end[S.n_slots]) ring_end[S.n_slots] = end;
        if (plan.lds > 160 * 1024 || plan.worker_lds > 160 * 1024) ++lds_over;
        if (S.net == LITE2) { ++lite2_rows; if (A.unit_pairs) ++lite2_pairs; }
        if (S.net == HEADS128 || S.net == HEADS256_64) { ++heads_rows; if (A.reg_tiles || plan.two_kernels) ++heads_reg; }
    }
    if (full) printf("%s", text.c_str());
}
typedef std::function<void(Setup &)> Change;
static void vary(const std::string &label, Setup S, const Change &change) { change(S); run(label, S); }

static const int SLOTS[] = {1, 16, 17, 24, 25, 46, 47, 83, 84, 96, 97, 119, 120, 128, 129, 148, 149, 176, 177, 200, 201, 224, 272, 400, 480, 544, 2048, 2049, 4096, 4097};

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--full")) full = true;
        else if (!strcmp(argv[i], "--roles")) roles = true;
        else if (!strcmp(argv[i], "--unit-regs")) unit_regs = true;
        else { fprintf(stderr, "usage: async_plan_table [--full | --roles | --unit-regs]\n"); return 2; }
    }
    clearenv();                                  // (the switches' defaults, not this shell's)
    default_switches = lrg_async_switches();
    if (unit_regs) printf("# label|gemv_units unit_pairs|unit_regs with LRG_ASYNC_UNIT_REGS unset, 0, 1|lds with it unset, 0, 1\n");
    else
    printf("%s\n", roles ? "# label|rt_head_every asked|rt_head_every rt_bb_every|CUs MIXED BRANCH2 BRANCH1 HEAD2|teams ring0 ring1 fill|fewest ring0 ring1 teams on 8 consecutive workgroups"
                         : COLUMNS);
    char l[128];

    // the paper's network on the whole chip: every slot count x the forms of the launch x units x teams
    for (int n : SLOTS)
        for (int bw : {0, 1, 4, 8, -1})
            for (int units : {0, -1})
                for (int teams = 0; teams <= 4; ++teams) {
                    snprintf(l, sizeof(l), "n%dw%du%dt%d", n, bw, units, teams);
                    vary(l, paper(n), [&](Setup &S) { S.ab.branch_waves = bw; S.ab.gemv_units = units; S.ab.teams = teams; });
                }
    // chips of other sizes (256 CUs: above; 1024: one where the largest slot counts have a plan)
    for (int cus : {304, 128, 64, 48, 1024})
        for (int n : SLOTS) {
            if (cus == 1024 && n < 4096) continue;
            snprintf(l, sizeof(l), "p13/c%d/n%d", cus, n);
            run(l, paper(n, cus));
        }
    // other networks, other set sizes
    for (int n : SLOTS) {
        snprintf(l, sizeof(l), "p9/n%d", n); run(l, make(n, 256, PAPER, 9, 512, 512));
        snprintf(l, sizeof(l), "p6/n%d", n); run(l, make(n, 256, PAPER, 6, 512, 512));
        snprintf(l, sizeof(l), "lite2/n%d", n); run(l, make(n, 256, LITE2, 13, 512, 512));
        snprintf(l, sizeof(l), "h128/n%d", n); run(l, make(n, 256, HEADS128, 13, 512, 512));
        snprintf(l, sizeof(l), "p13/32x64/n%d", n); run(l, make(n, 256, PAPER, 13, 32, 64));
    }
    // (behind the sweep above, whose order the golden table keeps: the paper's network but for the second head width -- the same C, the same P)
    for (int n : SLOTS) { snprintf(l, sizeof(l), "h256x64/n%d", n); run(l, make(n, 256, HEADS256_64, 13, 512, 512)); }

    // one argument at a time
    for (int n : {8, 68, 136, 272}) {
        const Setup B = paper(n);
        const std::string p = "n" + std::to_string(n) + "/";
        vary(p + "front_workgroups=20", B, [](Setup &S) { S.ab.front_workgroups = 20; });
        vary(p + "compute_units=128", B, [](Setup &S) { S.ab.compute_units = 128; });
        for (int parts : {1, 2, 4}) vary(p + "branch_parts=" + std::to_string(parts), B, [&](Setup &S) { S.ab.branch_parts = parts; });
        vary(p + "rows16=0", B, [](Setup &S) { S.ab.rows16 = 0; });
        vary(p + "gemv_units=1", B, [](Setup &S) { S.ab.gemv_units = 1; });
        // per-tile pool rows
        vary(p + "pool_rows/gemv_units=1", B, [](Setup &S) { grant_pool_rows(S); S.ab.gemv_units = 1; });
        vary(p + "pool_rows/small/gemv_units=1", B, [](Setup &S) { grant_pool_rows(S); S.ab.gemv_units = 1; S.ab.pool_rows_bytes -= 4; });
        vary(p + "pool_rows+8/gemv_units=1", B, [](Setup &S) { grant_pool_rows(S); S.ab.gemv_units = 1; S.ab.pool_rows = at<float>(R_POOL_ROWS, 8); });
        // speculation
        for (int k : {2, 3, 5, 16, 17}) vary(p + "speculate=" + std::to_string(k), B, [&](Setup &S) { S.ab.speculate = k; });
        // shared tail tiles
        vary(p + "tails", B, [](Setup &S) { grant_tails(S); });
        vary(p + "tails=48", B, [](Setup &S) { grant_tails(S, 48); });
        vary(p + "tails/tail_ctl+32", B, [](Setup &S) { grant_tails(S); S.ab.tail_ctl = at<int32_t>(R_TAIL_CTL, 32); });
        for (int us : {-1, 50}) vary(p + "tails/tail_close_us=" + std::to_string(us), B, [&](Setup &S) { grant_tails(S); S.ab.tail_close_us = us; });
        // in-launch fill-in
        for (int bw : {0, 4, 8, -1})
            for (int wgs : {0, 8}) {
                if (bw > 0 && wgs) continue;
                snprintf(l, sizeof(l), "fill/fill_wgs=%d/w%d", wgs, bw);
                vary(p + l, B, [&](Setup &S) { grant_fill(S, wgs); S.ab.branch_waves = bw; });
            }
        vary(p + "fill/w-1/t4", B, [](Setup &S) { grant_fill(S, 0); S.ab.branch_waves = -1; S.ab.teams = 4; });
        vary(p + "fill/fill_best+4", B, [](Setup &S) { grant_fill(S, 8); S.ab.fill_best = at<uint64_t>(R_FILL_BEST, 4); });
        vary(p + "fill/p9", make(n, 256, PAPER, 9, 512, 512), [](Setup &S) { grant_fill(S, 8); });
        // limits and counters
        vary(p + "start_wait_us=100", B, [](Setup &S) { S.ab.start_wait_us = 100; });
        vary(p + "budget_us=0", B, [](Setup &S) { S.budget_us = 0; });
        vary(p + "debug_ticks", B, [](Setup &S) { S.ab.debug_ticks = at<uint64_t>(R_DEBUG); });
        vary(p + "work=null", B, [](Setup &S) { S.ab.work = nullptr; });
    }
    vary("n48/speculate=3", paper(48), [](Setup &S) { S.ab.speculate = 3; });
    vary("n96/speculate=16", paper(96), [](Setup &S) { S.ab.speculate = 16; });
    vary("n264/speculate=2", paper(264), [](Setup &S) { S.ab.speculate = 2; });      // (132 groups: more than half of the CUs)
    vary("n68/front_workgroups=3", paper(68), [](Setup &S) { S.ab.front_workgroups = 3; });
    vary("n68/compute_units=200", paper(68), [](Setup &S) { S.ab.compute_units = 200; });
    vary("n68/speculate=2/work=null", paper(68), [](Setup &S) { S.ab.speculate = 2; S.ab.work = nullptr; });
    vary("n272/tails/gemv_units=-1", paper(272), [](Setup &S) { grant_tails(S); S.ab.gemv_units = -1; });
    vary("n272/tails/rows16=0", paper(272), [](Setup &S) { grant_tails(S); S.ab.rows16 = 0; });
    vary("n136/tails/pool_rows", paper(136), [](Setup &S) { grant_tails(S); grant_pool_rows(S); });
    vary("n272/fill/fill_wgs=500/w-1", paper(272), [](Setup &S) { grant_fill(S, 500); S.ab.branch_waves = -1; });
    vary("n68/fill/fill_rooms=2^18+1", paper(68), [](Setup &S) { grant_fill(S, 8); S.ab.fill_rooms = (1 << 18) + 1; });
    vary("n68/tails=2^25", paper(68), [](Setup &S) { grant_tails(S, 1 << 25); set_row_cap(S, S.b.row_cap + (1 << 25)); });

    // the switches, each at the values the plan tells apart, where it acts
    vary("n136/sw.unit_pairs=0", paper(136), [](Setup &S) { S.sw.unit_pairs = 0; });
    vary("n68/sw.unit_pairs=1", paper(68), [](Setup &S) { S.sw.unit_pairs = 1; });
    vary("n272/sw.unit_pairs=1", paper(272), [](Setup &S) { S.sw.unit_pairs = 1; });
    // (forced half-teams: granted to the paper's 1024 pooled features only, whatever the heads behind them)
    vary("lite2/n68/sw.unit_pairs=1", make(68, 256, LITE2, 13, 512, 512), [](Setup &S) { S.sw.unit_pairs = 1; });
    vary("lite2/n136/sw.unit_pairs=1", make(136, 256, LITE2, 13, 512, 512), [](Setup &S) { S.sw.unit_pairs = 1; });
    vary("h128/n68/sw.unit_pairs=1", make(68, 256, HEADS128, 13, 512, 512), [](Setup &S) { S.sw.unit_pairs = 1; });
    // (register tiles asked for by name, and wave-branch tasks: another head stack keeps the one-kernel launch)
    for (int bw : {1, 4}) {
        vary("h128/n68/w" + std::to_string(bw), make(68, 256, HEADS128, 13, 512, 512), [&](Setup &S) { S.ab.branch_waves = bw; });
        vary("h256x64/n68/w" + std::to_string(bw), make(68, 256, HEADS256_64, 13, 512, 512), [&](Setup &S) { S.ab.branch_waves = bw; });
    }
    for (int n : {200, 400}) {
        const std::string p = "n" + std::to_string(n) + "/";
        vary(p + "sw.gemv_batch=1/u-1", paper(n), [](Setup &S) { S.sw.gemv_batch = 1; S.ab.gemv_units = -1; });
        vary(p + "sw.gemv_batch=0/u-1", paper(n), [](Setup &S) { S.sw.gemv_batch = 0; S.ab.gemv_units = -1; });
        vary(p + "sw.gemv_batch=1/sw.gemv_batch_us=3.25/u-1", paper(n), [](Setup &S) { S.sw.gemv_batch = 1; S.sw.gemv_batch_us = 3.25; S.ab.gemv_units = -1; });
    }
    for (int n : {136, 272}) {
        const std::string p = "n" + std::to_string(n) + "/";
        vary(p + "tails/sw.tail_heads=0", paper(n), [](Setup &S) { grant_tails(S); S.sw.tail_heads = 0; });
        vary(p + "tails/sw.tail_heads=0/u-1", paper(n), [](Setup &S) { grant_tails(S); S.sw.tail_heads = 0; S.ab.gemv_units = -1; });
    }
    for (int n : {68, 136})
        for (int v : {0, 2}) vary("n" + std::to_string(n) + "/sw.rt_bb_every=" + std::to_string(v), paper(n), [&](Setup &S) { S.sw.rt_bb_every = v; });
    {
        const int n = 68;
        const std::string p = "n68/";
        vary(p + "sw.wave_fronts=20", paper(n), [](Setup &S) { S.sw.wave_fronts = 20; });
        vary(p + "sw.wave_fronts=20/front_workgroups=30", paper(n), [](Setup &S) { S.sw.wave_fronts = 20; S.ab.front_workgroups = 30; });
        vary(p + "sw.wave_fronts=20/w-1", paper(n), [](Setup &S) { S.sw.wave_fronts = 20; S.ab.branch_waves = -1; });
        vary(p + "sw.wave_extra_wgs=8", paper(n), [](Setup &S) { S.sw.wave_extra_wgs = 8; });
        vary(p + "sw.wave_wgs=40/w4", paper(n), [](Setup &S) { S.sw.wave_wgs = 40; S.ab.branch_waves = 4; });
        vary(p + "sw.wave_a_wgs=12/w4", paper(n), [](Setup &S) { S.sw.wave_a_wgs = 12; S.ab.branch_waves = 4; });
        vary(p + "sw.wave_split=8/w4", paper(n), [](Setup &S) { S.sw.wave_split = 8; S.ab.branch_waves = 4; });
        vary(p + "sw.rt_team_heads=1", paper(n), [](Setup &S) { S.sw.rt_team_heads = 1; });
    }
    for (int n : {68, 272}) {
        const std::string p = "n" + std::to_string(n) + "/";
        for (int teams : {2, 4}) {
            const std::string q = p + "w-1/t" + std::to_string(teams) + "/";
            vary(q + "fill/sw.fill_hybrid=0", paper(n), [&](Setup &S) { grant_fill(S, 0); S.ab.branch_waves = -1; S.ab.teams = teams; S.sw.fill_hybrid = 0; });
            for (int v : {-1, 1, 4}) vary(q + "sw.ring0_halves=" + std::to_string(v), paper(n), [&](Setup &S) { S.ab.branch_waves = -1; S.ab.teams = teams; S.sw.ring0_halves = v; });
            for (int v : {3, 23, 2}) vary(q + "sw.small_teams=" + std::to_string(v), paper(n), [&](Setup &S) { S.ab.branch_waves = -1; S.ab.teams = teams; S.sw.small_teams = v; });
        }
        vary(p + "w1/sw.ring0_halves=-1", paper(n), [](Setup &S) { S.ab.branch_waves = 1; S.sw.ring0_halves = -1; });
        vary(p + "w-1/t1/sw.ring0_halves=1", paper(n), [](Setup &S) { S.ab.branch_waves = -1; S.ab.teams = 1; S.sw.ring0_halves = 1; });
    }

    // one case per code of lrg_async_check, and the codes of the plan that the sweep above does not meet
    const Setup B = paper(68);
    vary("check/policy=3", B, [](Setup &S) { S.prm.policy = 3; });
    vary("check/max_steps=0", B, [](Setup &S) { S.max_steps = 0; });
    vary("check/weights.feature_size=9", B, [](Setup &S) { S.w.feature_size = 9; });
    vary("check/restarts=2", B, [](Setup &S) { S.prm.restarts = 2; });
    vary("check/max_points=2^17+1", B, [](Setup &S) { S.max_points = (1 << 17) + 1; });
    vary("check/queue=null", B, [](Setup &S) { S.ab.queue = nullptr; });
    vary("check/row_cap-small", B, [](Setup &S) { set_row_cap(S, 68 * 512 - 32); });
    vary("check/row_cap+8", B, [](Setup &S) { set_row_cap(S, S.b.row_cap + 8); });
    vary("check/queue_bytes-4", B, [](Setup &S) { S.ab.queue_bytes -= 4; });
    vary("check/queue+64", B, [](Setup &S) { S.ab.queue = at<int32_t>(R_QUEUE, 64); });
    run("check/n2^20", paper(1 << 20));
    vary("plan/packed=null", B, [](Setup &S) { S.w.packed = nullptr; });
    vary("plan/workspace_bytes-4", B, [](Setup &S) { S.b.workspace_bytes -= 4; });
    vary("plan/workspace+128", B, [](Setup &S) { S.b.workspace = at(R_WORKSPACE, 128); });
    vary("plan/n_head=2", B, [](Setup &S) { S.w.n_head = 2; S.w.head_ch[1] = 2; });
    vary("plan/conv1=128", make(68, 256, WIDE1, 13, 512, 512), [](Setup &) {});
    vary("plan/add_w0+8", B, [](Setup &S) { S.w.add_w[0] = at<float>(R_ADD_W, 8); });

    if (roles) return roles_bad;
    if (unit_regs) return unit_regs_bad;
    for (const auto &q : ring_end) printf("Q %d %lld %zu\n", q.first, q.second, lrg_grow_async_queue_bytes(q.first) / sizeof(int32_t));

    // what the sweep must hold
    int bad = 0;
    if (refused * 5 > rows) { fprintf(stderr, "async_plan_table: %d of %d rows are refusals: more than a fifth\n", refused, rows); bad = 1; }
    for (int code : {-20, -1, -2, -3, -4, -5, -6})
        if (!check_codes.count(LRG_EINVAL + code)) { fprintf(stderr, "async_plan_table: no case of lrg_async_check returns LRG_EINVAL - %d\n", -code); bad = 1; }
    for (int code : {-6, -7, -8, -9})
        if (!plan_codes.count(LRG_EINVAL + code)) { fprintf(stderr, "async_plan_table: no case of lrg_async_plan returns LRG_EINVAL - %d\n", -code); bad = 1; }
    // (the two gates of kernels written for the paper's shape only: half-teams in the units need 1024 pooled features -- lrg_async_gemv_unit2 -- and a two-kernel
    //  launch, with its register head tiles, the heads 256, 128, 2 -- lrg_team_head_tile_reg; no granted row of another network may show either)
    if (!lite2_rows || !heads_rows) { fprintf(stderr, "async_plan_table: no granted row of lite 2 / of another head stack on the paper's branches\n"); bad = 1; }
    if (lite2_pairs) { fprintf(stderr, "async_plan_table: %d lite-2 rows (512 pooled features) with unit_pairs 1\n", lite2_pairs); bad = 1; }
    if (heads_reg) { fprintf(stderr, "async_plan_table: %d rows of the heads 128, 64, 2 / 256, 64, 2 with a two-kernel launch\n", heads_reg); bad = 1; }
    if (lds_over) { fprintf(stderr, "async_plan_table: %d granted plans ask for more than 160 KB of LDS\n", lds_over); bad = 1; }
    for (int n : SLOTS)
        if (!ring_end.count(n)) { fprintf(stderr, "async_plan_table: no granted plan at %d slots\n", n); bad = 1; }
    return bad;
}
