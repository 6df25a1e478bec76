// The edge-classifier baseline of benchmarks.py (--mode edge, :308-353 and :418-436) for gfx950.  DESIGN §3.16.
//
// A batch of equalised rooms in the layout of lrg_baseline_segment (pts [n, ld >= 6], room_start, one linear-probe hash segment per
// room).  The 26 offsets are numbered in itertools.product order without the centre, so offsets o and 25 - o are opposite.  Edge {i, k}
// is stored once, in slot [i, o - 13] of the end i whose offset to k is one of 13 .. 25; per-edge arrays are [n, 13] float64, NaN where
// there is no neighbour.
//
//   lrg_edge_logits   init, insert, neighbours (the table nbr [n, 26], nmin / nmax [n, 6] of :333-339, the list of existing slots),
//                     then one lane per existing edge: the 30 float32 features of :309-324 and the four layers of the pickled
//                     MLPClassifier in float64, z [n, 13] = the logit.
//   lrg_edge_sigmoid  p = 1 / (1 + exp(-z)) on the device (the 'device' route; the 'host' route calls scipy's expit instead).
//   lrg_edge_segment  (on the workspace lrg_edge_logits prepared, or after preparing its own) from p [n, 13]: pmax per point and the 13-bit keep words (:346-352), the components of the kept edges
//                     (lrg_baseline_segment_mask, :406-416), and the fallback of :418-436 as independent searches:
//                       live      a second union over ALL voxel edges; a component is live when it holds a clustered point
//                       todo      the unlabelled points of live components (a dead component cannot change: it is not searched)
//                       search    one wavefront per search, lane o = the neighbour at offset o
//                       resolve   label[i] = label[stop[i]] along chains of decreasing index, by pointer jumping
//
// The MLP is a chain of rounded products and sums, acc = acc + x[k] * W[k][j] for k ascending from acc = 0, then the bias, then relu:
// no FMA, no MFMA, so that vectorised NumPy gives the same bits (tests/edge_ref.py) and the logit does not depend on the lane or the
// launch.  The weights are read at wave-uniform addresses (scalar loads through the constant cache); a lane holds its 30 inputs, the
// 50 accumulators of the second layer and the 25 of the third in registers and never stores an activation: hidden unit k of the
// first layer is computed when the second layer's k-th term needs it.
//
// The search (DESIGN §3.16 for the argument).  The reference's stack with duplicate pushes and mark-on-pop visits nodes in the order
// of a recursive DFS that takes the neighbours b of q in descending order of (p, b > q ? (1, b) : (0, offset of b from q)), each once.
// The search from i ends at the first node x != i that is clustered, or unlabelled with x < i (the reference has labelled it by then).
// The visited list and the stack (node, offset last taken) live in a slab of 3 search_cap words per wavefront; every lane performs the
// same stores to it, so a lane only ever reads words it has written itself.  A search that would visit more than search_cap nodes
// writes stop = -2 and is left to the caller.
//
// Visibility: as lrg_baselines.hip.  Parents by agent-scope atomics inside the union launch, the resolve pointers by agent-scope
// loads and stores inside a jump launch (any value read is a later node of the same chain), launch boundaries everywhere else.
#include "lrg_common.h"
#include "lrg_union.h"
#include "lrg_room_hash.h"

#define ED_THREADS 256
#define ED_SLOTS 13
#define ED_IN 30
#define ED_H1 100
#define ED_H2 50
#define ED_H3 25
// packed weights: W0 [30,100] | b0 [100] | W1 [100,50] | b1 [50] | W2 [50,25] | b2 [25] | W3 [25,1] | b3 [1], float64, [in, out] row-major
#define ED_W0 0
#define ED_B0 (ED_W0 + ED_IN * ED_H1)
#define ED_W1 (ED_B0 + ED_H1)
#define ED_B1 (ED_W1 + ED_H1 * ED_H2)
#define ED_W2 (ED_B1 + ED_H2)
#define ED_B2 (ED_W2 + ED_H2 * ED_H3)
#define ED_W3 (ED_B2 + ED_H3)
#define ED_B3 (ED_W3 + ED_H3)
#define ED_WEIGHTS (ED_B3 + 1)
#define ED_MAX_SEARCH_WAVES 2048
#define ED_MAX_SEARCH_CAP (1 << 20)

// scal words
enum { ED_STATUS = 0, ED_NEDGES = 1, ED_NTODO = 2, ED_DEAD = 4, ED_SEARCHES = 5, ED_OVERFLOW = 6, ED_VISITED = 7 };   // 4 .. 7: the counters, in the caller's order
enum { ED_ST_WINDOW = 1, ED_ST_DUPLICATE = 2, ED_ST_CHAIN = 4 };

struct LrgEdgeLayout {
    size_t scal, rooms, keys, vals, room_of, nbr, nmin, nmax, elist, logits_end;      // what lrg_edge_logits uses: independent of the rest
    size_t pmax, keepw, clab, parent, live, nxt, todo, slab, base;
    size_t base_bytes, total;
    long hslots;
    int waves;
};

static int ed_layout(int N, int R, int mcs, int cap, LrgEdgeLayout *L) {
    if (N < 0 || R < 0 || N > (1 << 26) || R > (1 << 20)) return LRG_EINVAL - 90;
    if (cap < 1 || cap > ED_MAX_SEARCH_CAP) return LRG_EINVAL - 91;
    L->hslots = lrg_room_hash_slots(N, R);
    L->waves = (N + 3) / 4 < ED_MAX_SEARCH_WAVES ? ((N + 3) / 4 + 3) / 4 * 4 : ED_MAX_SEARCH_WAVES;
    if (L->waves < 4) L->waves = 4;
    LrgArena ws;
    L->scal = ws.take(64 * 4);
    L->rooms = ws.take((size_t)(R + 1) * 4);
    L->keys = ws.take((size_t)L->hslots * 8);
    L->vals = ws.take((size_t)L->hslots * 4);
    L->room_of = ws.take((size_t)N * 4);
    L->nbr = ws.take((size_t)N * 26 * 4);
    L->nmin = ws.take((size_t)N * 6 * 4);
    L->nmax = ws.take((size_t)N * 6 * 4);
    L->elist = ws.take((size_t)N * ED_SLOTS * 4);
    L->logits_end = ws.total;
    L->pmax = ws.take((size_t)N * 8);
    L->keepw = ws.take((size_t)N * 4);
    L->clab = ws.take((size_t)N * 4);
    L->parent = ws.take((size_t)N * 4);
    L->live = ws.take((size_t)N * 4);
    L->nxt = ws.take((size_t)N * 4);
    L->todo = ws.take((size_t)N * 4);
    L->slab = ws.take((size_t)L->waves * 3 * (size_t)cap * 4);
    L->base_bytes = lrg_baseline_workspace_bytes(N, R, mcs);
    if (!L->base_bytes) return LRG_EINVAL - 92;
    L->base = ws.take(L->base_bytes);
    L->total = ws.total;
    return 0;
}

struct EdArgs {
    const float *pts; int ld;
    const int32_t *room_start; int n_rooms, n;
    float res;
    uint64_t *keys; int32_t *vals, *room_of, *nbr, *elist, *scal;
    long hslots;
    float *nmin, *nmax;
    double *z;                                     // logits: [n, 13] out
    const double *p; double rel, floor;            // segment: [n, 13] in
    double *pmax; uint32_t *keepw;
    int32_t *clab, *parent, *live, *nxt, *todo, *slab, *labels, *stop;
    int cap;
};

__global__ __launch_bounds__(ED_THREADS) void ed_init_kernel(EdArgs a) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < a.hslots) { a.keys[t] = LRG_HASH_EMPTY; a.vals[t] = -1; }
    if (t < 64) a.scal[t] = 0;
    if (t < a.n) a.room_of[t] = lrg_room_of(a.room_start, a.n_rooms, (int)t);
}

__global__ __launch_bounds__(ED_THREADS) void ed_insert_kernel(EdArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int r = a.room_of[i];
    int s, e;
    if (!lrg_room_bounds(a.room_start, a.n, r, &s, &e)) { a.room_of[i] = -1; return; }
    const float *p = a.pts + (long)i * a.ld;
    const uint64_t key = lrg_pack_voxel(lrg_voxel_of(p[0], a.res), lrg_voxel_of(p[1], a.res), lrg_voxel_of(p[2], a.res));
    if (key == LRG_HASH_EMPTY) { atomicOr(&a.scal[ED_STATUS], ED_ST_WINDOW); a.room_of[i] = -1; return; }
    uint64_t *keys; int32_t *vals; int mask;
    lrg_room_segment(a.keys, a.vals, r, s, e, &keys, &vals, &mask);
    if (!lrg_room_insert(keys, vals, mask, key, i)) atomicOr(&a.scal[ED_STATUS], ED_ST_DUPLICATE);      // the room is not equalised
}

// nbr [n, 26]; nmin / nmax over the point and its neighbours (:333-339: float32 minima and maxima, exact); the existing slots appended
// to elist (their order is not fixed and nothing depends on it); z [n, 13] = NaN when the caller wants logits
__global__ __launch_bounds__(ED_THREADS) void ed_neighbour_kernel(EdArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int cnt = 0;
    unsigned have = 0;
    if (i < a.n) {
        const int r = a.room_of[i];
        int s, e;
        const float *p = a.pts + (long)i * a.ld;
        float mn[6], mx[6];
        for (int c = 0; c < 6; ++c) mn[c] = mx[c] = p[c];
        const bool ok = r >= 0 && lrg_room_bounds(a.room_start, a.n, r, &s, &e);
        uint64_t *keys = nullptr; int32_t *vals = nullptr; int mask = 0;
        if (ok) lrg_room_segment(a.keys, a.vals, r, s, e, &keys, &vals, &mask);
        const int vx = lrg_voxel_of(p[0], a.res), vy = lrg_voxel_of(p[1], a.res), vz = lrg_voxel_of(p[2], a.res);
        int o = 0;
        for (int dx = -1; dx <= 1; ++dx)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dz = -1; dz <= 1; ++dz) {
                    if (!dx && !dy && !dz) continue;
                    const int k = ok ? lrg_hash_lookup(keys, vals, mask, lrg_pack_voxel(vx + dx, vy + dy, vz + dz)) : -1;
                    a.nbr[(long)i * 26 + o] = k;
                    if (k >= 0) {
                        const float *q = a.pts + (long)k * a.ld;
                        for (int c = 0; c < 6; ++c) { mn[c] = fminf(mn[c], q[c]); mx[c] = fmaxf(mx[c], q[c]); }
                        if (o >= 13) { have |= 1u << (o - 13); ++cnt; }
                    }
                    ++o;
                }
        for (int c = 0; c < 6; ++c) { a.nmin[(long)i * 6 + c] = mn[c]; a.nmax[(long)i * 6 + c] = mx[c]; }
        if (a.z) {
            const double nan = __longlong_as_double(0x7ff8000000000000LL);
            for (int s2 = 0; s2 < ED_SLOTS; ++s2) a.z[(long)i * ED_SLOTS + s2] = nan;
        }
    }
    // one atomic per wavefront
    const int incl = lrg_wave_incl_scan_i32(cnt);
    const int total = __builtin_amdgcn_readlane(incl, 63);
    int base = 0;
    if (lane == 0 && total) base = atomicAdd(&a.scal[ED_NEDGES], total);
    base = __builtin_amdgcn_readfirstlane(base);
    int at = base + incl - cnt;
    for (int s2 = 0; s2 < ED_SLOTS; ++s2)
        if (have & (1u << s2)) a.elist[at++] = i * ED_SLOTS + s2;
}

// One lane per existing edge: features, four layers, z.
__global__ __launch_bounds__(ED_THREADS) void ed_mlp_kernel(EdArgs a, const double *__restrict__ W) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.scal[ED_NEDGES]) return;
    const int slot = a.elist[t];
    const int i = slot / ED_SLOTS, s = slot - i * ED_SLOTS;
    const int k = a.nbr[(long)i * 26 + 13 + s];
    const float *p1 = a.pts + (long)i * a.ld, *p2 = a.pts + (long)k * a.ld;
    const float *mni = a.nmin + (long)i * 6, *mnk = a.nmin + (long)k * 6, *mxi = a.nmax + (long)i * 6, *mxk = a.nmax + (long)k * 6;
    double x[ED_IN];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float u = p1[2 + c], v = p2[2 + c];
        x[c] = (double)__fmul_rn(0.5f, __fadd_rn(u, v));
        x[4 + c] = (double)fminf(u, v);
        x[8 + c] = (double)fmaxf(u, v);
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const float u = p1[c], v = p2[c];
        x[12 + c] = (double)fabsf(__fsub_rn(u, v));
        x[18 + c] = (double)fmaxf(fabsf(__fsub_rn(u, mnk[c])), fabsf(__fsub_rn(v, mni[c])));
        x[24 + c] = (double)fmaxf(fabsf(__fsub_rn(u, mxk[c])), fabsf(__fsub_rn(v, mxi[c])));
    }
    double a2[ED_H2];
#pragma unroll
    for (int j = 0; j < ED_H2; ++j) a2[j] = 0.0;
#pragma unroll 1
    for (int u = 0; u < ED_H1; ++u) {              // hidden unit u of layer one, then its term of every layer-two sum
        double h = 0.0;
#pragma unroll
        for (int c = 0; c < ED_IN; ++c) h = __dadd_rn(h, __dmul_rn(x[c], W[ED_W0 + c * ED_H1 + u]));
        h = __dadd_rn(h, W[ED_B0 + u]);
        h = h > 0.0 ? h : 0.0;
#pragma unroll
        for (int j = 0; j < ED_H2; ++j) a2[j] = __dadd_rn(a2[j], __dmul_rn(h, W[ED_W1 + u * ED_H2 + j]));
    }
    double a3[ED_H3];
#pragma unroll
    for (int j = 0; j < ED_H3; ++j) a3[j] = 0.0;
#pragma unroll
    for (int u = 0; u < ED_H2; ++u) {
        double h = __dadd_rn(a2[u], W[ED_B1 + u]);
        h = h > 0.0 ? h : 0.0;
#pragma unroll
        for (int j = 0; j < ED_H3; ++j) a3[j] = __dadd_rn(a3[j], __dmul_rn(h, W[ED_W2 + u * ED_H3 + j]));
    }
    double zz = 0.0;
#pragma unroll
    for (int u = 0; u < ED_H3; ++u) {
        double h = __dadd_rn(a3[u], W[ED_B2 + u]);
        h = h > 0.0 ? h : 0.0;
        zz = __dadd_rn(zz, __dmul_rn(h, W[ED_W3 + u]));
    }
    a.z[slot] = __dadd_rn(zz, W[ED_B3]);
}

__global__ __launch_bounds__(ED_THREADS) void ed_sigmoid_kernel(const double *z, long m, double *p) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m) return;
    const double v = z[t];
    p[t] = v == v ? 1.0 / (1.0 + exp(-v)) : v;
}

// the probability of the edge from q to its neighbour at offset o (the neighbour exists)
__device__ __forceinline__ double ed_prob(const EdArgs &a, int q, int o, int b) {
    return o >= 13 ? a.p[(long)q * ED_SLOTS + o - 13] : a.p[(long)b * ED_SLOTS + 12 - o];
}

// :346-350: the maximum of 0 and the probabilities of the point's edges
__global__ __launch_bounds__(ED_THREADS) void ed_pmax_kernel(EdArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    double m = 0.0;
    for (int o = 0; o < 26; ++o) {
        const int b = a.nbr[(long)i * 26 + o];
        if (b < 0) continue;
        const double p = ed_prob(a, i, o, b);
        m = p > m ? p : m;
    }
    a.pmax[i] = m;
}

// :351-352 for the 13 slots of the point; also the fields the later launches start from
__global__ __launch_bounds__(ED_THREADS) void ed_keep_kernel(EdArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    unsigned w = 0;
    const double ti = __dmul_rn(a.rel, a.pmax[i]);
    for (int s = 0; s < ED_SLOTS; ++s) {
        const int k = a.nbr[(long)i * 26 + 13 + s];
        if (k < 0) continue;
        const double p = a.p[(long)i * ED_SLOTS + s];
        if (p > ti && p > __dmul_rn(a.rel, a.pmax[k]) && p > a.floor) w |= 1u << s;
    }
    if (i == 0) a.scal[ED_NTODO] = a.scal[ED_DEAD] = a.scal[ED_SEARCHES] = a.scal[ED_OVERFLOW] = a.scal[ED_VISITED] = 0;   // a prepared workspace keeps its status
    a.keepw[i] = w;
    a.parent[i] = i;
    a.live[i] = 0;
    a.stop[i] = -1;
}

// every voxel edge, each once
__global__ __launch_bounds__(ED_THREADS) void ed_union_all_kernel(EdArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    for (int o = 0; o < 26; ++o) {
        const int k = a.nbr[(long)i * 26 + o];
        if (k >= 0 && k < i) bl_union(a.parent, i, k);
    }
}

__global__ __launch_bounds__(ED_THREADS) void ed_live_kernel(EdArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int root = bl_find(a.parent, i);
    __hip_atomic_store(a.parent + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a.clab[i] > 0) a.live[root] = 1;           // every writer writes 1; read after the launch
}

// the searches to run; the terminal label and the identity pointer of every point
__global__ __launch_bounds__(ED_THREADS) void ed_todo_kernel(EdArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int want = 0, dead = 0;
    if (i < a.n) {
        const int lab = a.clab[i];
        const int alive = a.live[a.parent[i]];
        want = lab == 0 && alive;
        dead = lab == 0 && !alive;
        a.labels[i] = lab;
        a.nxt[i] = i;
    }
    const unsigned long long bw = __ballot(want), bd = __ballot(dead);
    int base = 0;
    if (lane == 0) {
        if (bw) base = atomicAdd(&a.scal[ED_NTODO], __popcll(bw));
        if (bd) atomicAdd(&a.scal[ED_DEAD], __popcll(bd));
    }
    base = __builtin_amdgcn_readfirstlane(base);
    if (want) a.todo[base + __popcll(bw & ((1ULL << lane) - 1))] = i;
}

__device__ __forceinline__ long long ed_wave_max_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}

// wave-uniform values are made scalars (readfirstlane / readlane), so that every branch of the search is a scalar branch and every
// cross-lane operation runs with all 64 lanes: the compiler cannot prove that a value loaded from the slab is the same in every lane
#define ED_UNI(v) __builtin_amdgcn_readfirstlane(v)

__global__ __launch_bounds__(ED_THREADS) void ed_search_kernel(EdArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = ED_UNI((int)(((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const int nwaves = (int)gridDim.x * (ED_THREADS / 64);
    const int cap = a.cap;
    int32_t *vis = a.slab + (long)wave * 3 * (long)cap, *stk = vis + cap, *cur = stk + cap;
    const int ntodo = ED_UNI(a.scal[ED_NTODO]);
    for (int t = wave; t < ntodo; t += nwaves) {
        const int i = ED_UNI(a.todo[t]);
        int nv = 1, top = 1, result = -1;
        vis[0] = i; stk[0] = i; cur[0] = -1;       // every lane stores the same words (see the header comment)
        while (top > 0) {
            const int q = ED_UNI(stk[top - 1]), last = ED_UNI(cur[top - 1]);
            int b = -1;
            long long pb = -1;
            int tie = 0;
            if (lane < 26) {
                b = a.nbr[(long)q * 26 + lane];
                if (b >= 0) {
                    pb = __double_as_longlong(ed_prob(a, q, lane, b));       // p >= 0: the bit pattern orders as the value
                    tie = b > q ? (1 << 28) + b : lane;
                }
            }
            bool valid = b >= 0;
            if (last >= 0) {
                const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(unsigned long long)pb, last);
                const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)pb >> 32), last);
                const long long lpb = (long long)(((unsigned long long)hi << 32) | lo);
                const int ltie = __builtin_amdgcn_readlane(tie, last);
                valid = valid && (pb < lpb || (pb == lpb && tie < ltie));
            }
            const long long best = ed_wave_max_i64(valid ? pb : LLONG_MIN);
            const bool cand = valid && pb == best;
            const unsigned bt = lrg_wave_max_u32(cand ? (unsigned)tie + 1u : 0u);
            if (bt == 0) { --top; continue; }                                  // q's neighbours are used up
            const unsigned long long pick = __ballot(cand && (unsigned)tie + 1u == bt);
            const int slot = __ffsll((long long)pick) - 1;
            const int x = __builtin_amdgcn_readlane(b, slot);
            cur[top - 1] = slot;
            bool seen = false;
            for (int j0 = 0; j0 < nv && !seen; j0 += 64) {
                const int j = j0 + lane;
                seen = __ballot(j < nv && vis[j] == x) != 0;
            }
            if (seen) continue;
            if (ED_UNI(a.clab[x]) > 0 || x < i) { result = x; break; }
            if (nv >= cap) { result = -2; break; }
            vis[nv] = x; stk[top] = x; cur[top] = -1;
            ++nv; ++top;
        }
        if (lane == 0) {
            a.stop[i] = result;
            atomicAdd(&a.scal[ED_SEARCHES], 1);
            if (result == -2) atomicAdd(&a.scal[ED_OVERFLOW], 1);
            atomicMax(&a.scal[ED_VISITED], nv);
        }
    }
}

// nxt[i] = the unlabelled point the search stopped at, or i with the cluster's label when it stopped at a clustered point
__global__ __launch_bounds__(ED_THREADS) void ed_link_kernel(EdArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int x = a.stop[i];
    if (x < 0) return;
    const int lab = a.clab[x];
    if (lab > 0) a.labels[i] = lab; else a.nxt[i] = x;
}

__global__ __launch_bounds__(ED_THREADS) void ed_jump_kernel(EdArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int r = bl_load(a.nxt + i);
    if (r == i) return;
    const int rr = bl_load(a.nxt + r);
    if (rr != r) __hip_atomic_store(a.nxt + i, rr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the label of the chain's end (a point with nxt = itself, whose label no lane of this launch writes)
__global__ __launch_bounds__(ED_THREADS) void ed_resolve_kernel(EdArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int r = a.nxt[i];
    if (r == i) return;
    if (a.nxt[r] != r) { atomicOr(&a.scal[ED_STATUS], ED_ST_CHAIN); return; }
    a.labels[i] = a.labels[r];
}

// the checks and the argument block that the two entries share; room_start is copied to the workspace on the stream
static int ed_setup(const float *pts, int ld, const int32_t *room_start, int n_rooms, float resolution, int mcs, int cap, void *ws, size_t ws_bytes,
                    bool logits_only, hipStream_t st, LrgEdgeLayout *L, EdArgs *out) {
    if (n_rooms < 1 || n_rooms > (1 << 20) || !room_start || room_start[0] != 0) return LRG_EINVAL - 93;
    for (int r = 0; r < n_rooms; ++r)
        if (room_start[r + 1] < room_start[r]) return LRG_EINVAL - 93;
    const int n = room_start[n_rooms];
    int rc = ed_layout(n, n_rooms, mcs, cap, L);
    if (rc) return rc;
    if (!ws || ((uintptr_t)ws & 255) || ws_bytes < (logits_only ? L->logits_end : L->total)) return LRG_EINVAL - 95;
    if (n > 0 && (!pts || ld < 6)) return LRG_EINVAL - 93;
    if (!(resolution > 0.f)) return LRG_EINVAL - 96;
    char *w = static_cast<char *>(ws);
    EdArgs a = {};
    int32_t *rooms = reinterpret_cast<int32_t *>(w + L->rooms);
    LRG_HIP_CHECK(hipMemcpyAsync(rooms, room_start, (size_t)(n_rooms + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
    a.pts = pts; a.ld = ld; a.room_start = rooms; a.n_rooms = n_rooms; a.n = n; a.res = resolution;
    a.keys = reinterpret_cast<uint64_t *>(w + L->keys); a.vals = reinterpret_cast<int32_t *>(w + L->vals);
    a.room_of = reinterpret_cast<int32_t *>(w + L->room_of); a.nbr = reinterpret_cast<int32_t *>(w + L->nbr);
    a.elist = reinterpret_cast<int32_t *>(w + L->elist); a.scal = reinterpret_cast<int32_t *>(w + L->scal);
    a.nmin = reinterpret_cast<float *>(w + L->nmin); a.nmax = reinterpret_cast<float *>(w + L->nmax);
    a.hslots = L->hslots; a.cap = cap;
    if (!logits_only) {
        a.pmax = reinterpret_cast<double *>(w + L->pmax); a.keepw = reinterpret_cast<uint32_t *>(w + L->keepw);
        a.clab = reinterpret_cast<int32_t *>(w + L->clab); a.parent = reinterpret_cast<int32_t *>(w + L->parent);
        a.live = reinterpret_cast<int32_t *>(w + L->live); a.nxt = reinterpret_cast<int32_t *>(w + L->nxt);
        a.todo = reinterpret_cast<int32_t *>(w + L->todo); a.slab = reinterpret_cast<int32_t *>(w + L->slab);
    }
    *out = a;
    return 0;
}

static inline int ed_grid(long m) { return (int)((m + ED_THREADS - 1) / ED_THREADS); }

// init, insert, neighbours
static void ed_prepare(const EdArgs &a, hipStream_t st) {
    const long init_n = a.hslots > (long)a.n + 64 ? a.hslots : (long)a.n + 64;
    hipLaunchKernelGGL(ed_init_kernel, dim3(ed_grid(init_n)), dim3(ED_THREADS), 0, st, a);
    if (a.n > 0) {
        hipLaunchKernelGGL(ed_insert_kernel, dim3(ed_grid(a.n)), dim3(ED_THREADS), 0, st, a);
        hipLaunchKernelGGL(ed_neighbour_kernel, dim3(ed_grid(a.n)), dim3(ED_THREADS), 0, st, a);
    }
}

extern "C" {

size_t lrg_edge_workspace_bytes(int n_points, int n_rooms, int min_cluster_size, int search_cap) {
    LrgEdgeLayout L;
    if (ed_layout(n_points, n_rooms, min_cluster_size, search_cap, &L)) return 0;
    return L.total;
}

int lrg_edge_logits(const float *pts, int ld, const int32_t *room_start, int n_rooms, float resolution, const double *weights, void *ws,
                    size_t ws_bytes, double *z, float *nmin, float *nmax, void *stream) {
    LrgEdgeLayout L;
    EdArgs a;
    hipStream_t st = (hipStream_t)stream;
    int rc = ed_setup(pts, ld, room_start, n_rooms, resolution, 1, 1, ws, ws_bytes, true, st, &L, &a);
    if (rc) return rc;
    if (!weights || (a.n > 0 && !z)) return LRG_EINVAL - 94;
    a.z = z;
    ed_prepare(a, st);
    if (a.n > 0) {
        hipLaunchKernelGGL(ed_mlp_kernel, dim3(ed_grid((long)a.n * ED_SLOTS)), dim3(ED_THREADS), 0, st, a, weights);
        if (nmin) LRG_HIP_CHECK(hipMemcpyAsync(nmin, a.nmin, (size_t)a.n * 6 * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (nmax) LRG_HIP_CHECK(hipMemcpyAsync(nmax, a.nmax, (size_t)a.n * 6 * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    LRG_LAUNCH_CHECK();
    return 0;
}

int lrg_edge_sigmoid(const double *z, long count, double *p, void *stream) {
    if (count < 0 || count > (long)ED_SLOTS << 26) return LRG_EINVAL - 97;
    if (count == 0) return 0;
    if (!z || !p) return LRG_EINVAL - 97;
    hipLaunchKernelGGL(ed_sigmoid_kernel, dim3(ed_grid(count)), dim3(ED_THREADS), 0, (hipStream_t)stream, z, count, p);
    LRG_LAUNCH_CHECK();
    return 0;
}

int lrg_edge_segment(const float *pts, int ld, const int32_t *room_start, int n_rooms, float resolution, const double *p, double rel, double floor,
                     int min_cluster_size, int search_cap, void *ws, size_t ws_bytes, int32_t *labels, int32_t *n_clusters, int32_t *stop,
                     int32_t *counters, uint32_t *keep, int32_t *cluster_labels, int prepared, void *stream) {
    LrgEdgeLayout L;
    EdArgs a;
    hipStream_t st = (hipStream_t)stream;
    int rc = ed_setup(pts, ld, room_start, n_rooms, resolution, min_cluster_size, search_cap, ws, ws_bytes, false, st, &L, &a);
    if (rc) return rc;
    if (!labels || !n_clusters || !stop || !counters || (a.n > 0 && !p)) return LRG_EINVAL - 94;
    if (!(rel >= 0.0) || !(floor == floor)) return LRG_EINVAL - 98;
    a.p = p; a.rel = rel; a.floor = floor; a.labels = labels; a.stop = stop;
    a.z = nullptr;
    if (!prepared) ed_prepare(a, st);              // else: the workspace is as lrg_edge_logits left it for these rooms
    const int gn = ed_grid(a.n);
    if (a.n > 0) {
        hipLaunchKernelGGL(ed_pmax_kernel, dim3(gn), dim3(ED_THREADS), 0, st, a);
        hipLaunchKernelGGL(ed_keep_kernel, dim3(gn), dim3(ED_THREADS), 0, st, a);
    }
    rc = lrg_baseline_segment_mask(pts, ld, room_start, n_rooms, resolution, a.keepw, min_cluster_size, static_cast<char *>(ws) + L.base, L.base_bytes,
                                   a.clab, n_clusters, stream);
    if (rc) return rc;
    if (a.n > 0) {
        hipLaunchKernelGGL(ed_union_all_kernel, dim3(gn), dim3(ED_THREADS), 0, st, a);
        hipLaunchKernelGGL(ed_live_kernel, dim3(gn), dim3(ED_THREADS), 0, st, a);
        hipLaunchKernelGGL(ed_todo_kernel, dim3(gn), dim3(ED_THREADS), 0, st, a);
        hipLaunchKernelGGL(ed_search_kernel, dim3(L.waves / 4), dim3(ED_THREADS), 0, st, a);
        hipLaunchKernelGGL(ed_link_kernel, dim3(gn), dim3(ED_THREADS), 0, st, a);
        int passes = 1;                                // a chain has fewer than n links: ceil(log2 n) doublings
        while ((1L << passes) < a.n) ++passes;
        for (int k = 0; k < passes; ++k) hipLaunchKernelGGL(ed_jump_kernel, dim3(gn), dim3(ED_THREADS), 0, st, a);
        hipLaunchKernelGGL(ed_resolve_kernel, dim3(gn), dim3(ED_THREADS), 0, st, a);
        if (keep) LRG_HIP_CHECK(hipMemcpyAsync(keep, a.keepw, (size_t)a.n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        if (cluster_labels) LRG_HIP_CHECK(hipMemcpyAsync(cluster_labels, a.clab, (size_t)a.n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    }
    LRG_HIP_CHECK(hipMemcpyAsync(counters, a.scal + ED_DEAD, 4 * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    LRG_LAUNCH_CHECK();
    return 0;
}

int lrg_edge_status(const void *ws, int32_t *host_status, void *stream) {
    if (!ws || !host_status) return LRG_EINVAL - 93;
    LRG_HIP_CHECK(hipMemcpyAsync(host_status, ws, sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));   // scal is the workspace's first word
    LRG_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

}  // extern "C"
