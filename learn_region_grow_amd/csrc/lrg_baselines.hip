// The classical region-growing baselines of benchmarks.py (modes normal, curvature, color, feature, smoothness) for gfx950.
//
// Every mode puts edges on the 26-neighbour voxel graph of an equalised room with a per-mode predicate (benchmarks.py:251-378)
// and labels the connected components of more than min_cluster_size points (:380-416).  Here a batch of rooms goes through a
// fixed sequence of launches, one thread per point in each:
//   init     hash slots empty, parent[i] = i, counters cleared, the room of every point (binary search in room_start)
//   insert   voxel key -> the room's own linear-probe segment (lrg_pack_voxel / lrg_fmix64); a key met twice is an error
//   union    26 lookups, the predicate, then a lock-free union of i and j for the neighbours j < i (every predicate is
//            symmetric, so each edge is handled once).  The larger root is linked under the smaller by CAS, so the root
//            of a component is its minimum index whatever the order of the unions.
//   count    every point's root (path halving), component sizes, and for smoothness the minimum (rank, index) of each
//   keep     one lane per component root: the keep decision (size > min_cluster_size; for smoothness a component of
//            2 .. min_cluster_size points replays the reference's DFS, whose pop count counts duplicates) and flag[key] = 1,
//            key = the root's position in its room (networkx's order) or the smallest rank (smoothness)
//   scan     exclusive scan of the flags (three launches); per-room ids are differences of the global scan
//   label    label[i] = scan[key of i's component] - scan[room start] + 1 if kept, else 0; n_clusters per room
//
// lrg_baseline_segment_fpfh (benchmarks.py --mode fpfh) puts one launch in front of these: the normalised histograms
// u [n, 33] in float64, which its edge predicate reads; the descriptor itself is lrg_fpfh.hip's.
//
// lrg_baseline_segment_mask (benchmarks.py --mode edge) runs the same launches on edges the caller has decided: a 13-bit
// word per point, bit s = the edge to the neighbour at offset 13 + s (the positive half of the 26 offsets) is kept.
//
// Features solved on the device (DESIGN §3.8 "verified"): lrg_baseline_eig is prep_jacobi3 on every covariance with a bound on each
// value's distance from LAPACK's, and lrg_baseline_certify (init, insert, certify, tally) flags both ends of every edge whose
// predicate could come out differently within those bounds, so that only they go through LAPACK on the host.
//
// Visibility (MI355X: per-XCD L2s are not coherent).  Inside the union launch every parent word is read with an agent-scope
// relaxed atomic load (global_load sc1: never from a stale L1) and changed only by agent-scope CAS, which is performed at the
// device's coherence point.  Correctness needs only that CAS: parents only ever decrease, so a value read late is still an
// ancestor of the word's point (a larger one), and a root seen as a root that is no longer one fails its CAS and the loop
// continues from the value the CAS returned.  Every other cross-workgroup read (hash values, final parents, sizes, keys,
// flags, scans) is separated from its writes by a launch boundary.
#include "lrg_common.h"
#include "lrg_eig3.h"
#include "lrg_union.h"
#include "lrg_room_hash.h"

#define BL_THREADS 256

enum { BL_NORMAL = 0, BL_CURVATURE = 1, BL_COLOR = 2, BL_FEATURE = 3, BL_SMOOTHNESS = 4, BL_EMBEDDING = 5, BL_LABELS = 6, BL_FPFH = 7, BL_MASK = 8 };   // 5: lrg_baseline_segment_embedding only, 6: lrg_baseline_segment_labels only, 7: lrg_baseline_segment_fpfh only, 8: lrg_baseline_segment_mask only
// status bits (lrg_baseline_status)
enum { BL_ST_WINDOW = 1, BL_ST_DUPLICATE = 2, BL_ST_RANK = 4, BL_ST_STACK = 8 };

struct LrgBaselineLayout {
    size_t keys, vals;                 // the rooms' hash segments (lrg_room_hash.h)
    size_t rooms, room_of, parent, size, minkey, ckey, visited, flag, scan, bsum, stack, scal;
    size_t total;
    long hslots, stack_cap;
};

static int bl_layout(int N, int R, int mcs, LrgBaselineLayout *L) {
    if (N < 0 || R < 0 || N > (1 << 26) || R > (1 << 20)) return LRG_EINVAL - 70;
    if (mcs < 1 || mcs > LRG_BASELINE_MAX_MIN_CLUSTER) return LRG_EINVAL - 71;
    L->hslots = lrg_room_hash_slots(N, R);
    // a replayed component of c <= mcs points pushes at most 26 c times (only a point's first pop finds unvisited
    // neighbours): 1 + 26 c entries each, at most 27 n over all components
    L->stack_cap = 27L * N;
    LrgArena ws;
    L->keys = ws.take((size_t)L->hslots * 8);
    L->vals = ws.take((size_t)L->hslots * 4);
    L->rooms = ws.take((size_t)(R + 1) * 4);
    L->room_of = ws.take((size_t)N * 4);
    L->parent = ws.take((size_t)N * 4);
    L->size = ws.take((size_t)N * 4);
    L->minkey = ws.take((size_t)N * 8);
    L->ckey = ws.take((size_t)N * 4);
    L->visited = ws.take((size_t)N * 4);
    L->flag = ws.take((size_t)(N + 1) * 4);
    L->scan = ws.take((size_t)(N + 1) * 4);
    L->bsum = ws.take((size_t)(lrg_scan_blocks(N + 1) + 1) * 4);
    L->stack = ws.take((size_t)L->stack_cap * 4);
    L->scal = ws.take(64 * 4);
    L->total = ws.total;
    return 0;
}

struct BlArgs {
    const float *pts; int ld;
    const int32_t *room_start; int n_rooms, n;
    float res; int mode;
    const double *normals, *curv; const int32_t *rank;
    const float *emb; int dim;
    const int32_t *cls;
    const uint32_t *keep;                                              // lrg_baseline_segment_mask only: [n] 13-bit keep words
    double *unit;                                                      // lrg_baseline_segment_fpfh only: [n, 33] normalised histograms
    double t1, t2, t3; int mcs;
    uint64_t *keys; int32_t *vals, *room_of, *parent, *size; unsigned long long *minkey;
    int32_t *ckey, *visited, *flag, *scan, *bsum, *stack, *scal;
    long hslots, stack_cap;
    int32_t *labels, *n_clusters;
    const double *nslack, *cslack; int32_t *cflags, *n_flagged;       // lrg_baseline_certify only (NULL otherwise)
};

// normals[k].dot(normals[i]) as OpenBLAS's ddot computes it for n = 3: fma(a2, b2, fma(a1, b1, a0 * b0))
__device__ __forceinline__ double bl_normal_dot(const double *nrm, int i, int k) {
    const double *a = nrm + 3L * k, *b = nrm + 3L * i;
    return __fma_rn(a[2], b[2], __fma_rn(a[1], b[1], __dmul_rn(a[0], b[0])));
}
__device__ __forceinline__ bool bl_normal_edge(const double *nrm, int i, int k, double t) { return bl_normal_dot(nrm, i, k) > t; }

// abs(curvatures[k] - curvatures[i]) < t in float64
__device__ __forceinline__ double bl_curv_diff(const double *c, int i, int k) { return fabs(__dsub_rn(c[k], c[i])); }
__device__ __forceinline__ bool bl_curv_edge(const double *c, int i, int k, double t) { return bl_curv_diff(c, i, k) < t; }

// numpy.sum((p[k,3:6] - p[i,3:6])**2) < t on float32 rows: squares rounded to float32, summed (d0 + d1) + d2, compared with
// float32(t) (NumPy 2 casts the Python float to the array's dtype).  No contraction.
__device__ __forceinline__ bool bl_color_edge(const float *pts, int ld, int i, int k, float t) {
    const float *p = pts + (long)k * ld + 3, *q = pts + (long)i * ld + 3;
    const float d0 = __fsub_rn(p[0], q[0]), d1 = __fsub_rn(p[1], q[1]), d2 = __fsub_rn(p[2], q[2]);
    const float s = __fadd_rn(__fadd_rn(__fmul_rn(d0, d0), __fmul_rn(d1, d1)), __fmul_rn(d2, d2));
    return s < t;
}

// emb[k].dot(emb[i]) > t (test_mcpnet.py:131): float64 copies of float32 values, so every product is exact; summed in order
// ((p0 + p1) + p2) + ... as OpenBLAS's ddot does for n = 10.  Symmetric in i and k.
__device__ __forceinline__ bool bl_embedding_edge(const float *emb, int dim, int i, int k, double t) {
    const float *a = emb + (long)k * dim, *b = emb + (long)i * dim;
    double d = __dmul_rn((double)a[0], (double)b[0]);
    for (int c = 1; c < dim; ++c) d = __dadd_rn(d, __dmul_rn((double)a[c], (double)b[c]));
    return d > t;
}

// u[k].dot(u[i]) > t on the normalised histograms (benchmarks.py:359-366), summed in order, every product and sum rounded; a NaN
// (zero histogram) is no edge.  Symmetric in i and k.
#define BL_FPFH_DIM 33
__device__ __forceinline__ bool bl_fpfh_edge(const double *u, int i, int k, double t) {
    const double *a = u + (long)k * BL_FPFH_DIM, *b = u + (long)i * BL_FPFH_DIM;
    double d = __dmul_rn(a[0], b[0]);
    for (int c = 1; c < BL_FPFH_DIM; ++c) d = __dadd_rn(d, __dmul_rn(a[c], b[c]));
    return d > t;
}

// unit[i] = double(hist[i]) / sqrt(sum of its squares taken in order); 0 / 0 = NaN for a zero histogram
__global__ __launch_bounds__(BL_THREADS) void bl_fpfh_unit_kernel(const float *hist, int n, double *unit) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *h = hist + (long)i * BL_FPFH_DIM;
    double s = 0.0;
    for (int c = 0; c < BL_FPFH_DIM; ++c) s = __dadd_rn(s, __dmul_rn((double)h[c], (double)h[c]));
    const double nrm = __dsqrt_rn(s);
    for (int c = 0; c < BL_FPFH_DIM; ++c) unit[(long)i * BL_FPFH_DIM + c] = __ddiv_rn((double)h[c], nrm);
}

// the caller's decision on the edge from i to its neighbour k at offset o (0 .. 25 in itertools.product order without the centre;
// o and 25 - o are opposite): the edge is stored once, at the end whose offset to the other is one of 13 .. 25, as bit o - 13
__device__ __forceinline__ bool bl_mask_edge(const uint32_t *keep, int i, int k, int o) {
    return o >= 13 ? (keep[i] >> (o - 13)) & 1u : (keep[k] >> (12 - o)) & 1u;
}

__device__ __forceinline__ bool bl_edge(const BlArgs &a, int i, int k, int o) {
    switch (a.mode) {
    case BL_MASK: return bl_mask_edge(a.keep, i, k, o);
    case BL_NORMAL: case BL_SMOOTHNESS: return bl_normal_edge(a.normals, i, k, a.t1);
    case BL_CURVATURE: return bl_curv_edge(a.curv, i, k, a.t1);
    case BL_COLOR: return bl_color_edge(a.pts, a.ld, i, k, (float)a.t1);
    case BL_EMBEDDING: return bl_embedding_edge(a.emb, a.dim, i, k, a.t1);
    case BL_LABELS: return a.cls[k] == a.cls[i];             // class_labels[voxel_map[kk]] == class_labels[i] (benchmarks.py:305)
    case BL_FPFH: return bl_fpfh_edge(a.unit, i, k, a.t1);
    default:
        return bl_normal_edge(a.normals, i, k, a.t1) && bl_curv_edge(a.curv, i, k, a.t2) &&
               bl_color_edge(a.pts, a.ld, i, k, (float)a.t3);
    }
}


__global__ __launch_bounds__(BL_THREADS) void bl_init_kernel(BlArgs a) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < a.hslots) { a.keys[t] = LRG_HASH_EMPTY; a.vals[t] = -1; }
    if (t < 64) a.scal[t] = 0;
    if (t <= a.n) a.flag[t] = 0;
    if (a.cflags) {
        if (t < a.n) a.cflags[t] = 0;
        if (t == 0) *a.n_flagged = 0;
    }
    if (t >= a.n) return;
    const int i = (int)t;
    a.room_of[i] = lrg_room_of(a.room_start, a.n_rooms, i);
    a.parent[i] = i;
    a.size[i] = 0;
    a.minkey[i] = ~0ULL;
    a.ckey[i] = -1;
    a.visited[i] = 0;
}

__device__ __forceinline__ uint64_t bl_key(const BlArgs &a, int i, int dx, int dy, int dz) {
    const float *p = a.pts + (long)i * a.ld;
    return lrg_pack_voxel(lrg_voxel_of(p[0], a.res) + dx, lrg_voxel_of(p[1], a.res) + dy, lrg_voxel_of(p[2], a.res) + dz);
}

__global__ __launch_bounds__(BL_THREADS) void bl_insert_kernel(BlArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int r = a.room_of[i];
    int s, e;
    if (!lrg_room_bounds(a.room_start, a.n, r, &s, &e)) return;
    const uint64_t key = bl_key(a, i, 0, 0, 0);
    if (key == LRG_HASH_EMPTY) { atomicOr(&a.scal[0], BL_ST_WINDOW); a.room_of[i] = -1; return; }
    uint64_t *keys; int32_t *vals; int mask;
    lrg_room_segment(a.keys, a.vals, r, s, e, &keys, &vals, &mask);
    if (!lrg_room_insert(keys, vals, mask, key, i)) atomicOr(&a.scal[0], BL_ST_DUPLICATE);      // the room is not equalised
}

__global__ __launch_bounds__(BL_THREADS) void bl_union_kernel(BlArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int r = a.room_of[i];
    if (r < 0) return;
    int s, e;
    if (!lrg_room_bounds(a.room_start, a.n, r, &s, &e)) return;
    uint64_t *keys; int32_t *vals; int mask;
    lrg_room_segment(a.keys, a.vals, r, s, e, &keys, &vals, &mask);
    const float *p = a.pts + (long)i * a.ld;
    const int vx = lrg_voxel_of(p[0], a.res), vy = lrg_voxel_of(p[1], a.res), vz = lrg_voxel_of(p[2], a.res);
    int o = 0;                                     // the offset's number, the centre left out
    for (int dx = -1; dx <= 1; ++dx)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dz = -1; dz <= 1; ++dz) {
                if (!dx && !dy && !dz) continue;
                const int at = o++;
                const int k = lrg_hash_lookup(keys, vals, mask, lrg_pack_voxel(vx + dx, vy + dy, vz + dz));
                if (k < 0 || k >= i) continue;
                if (bl_edge(a, i, k, at)) bl_union(a.parent, i, k);
            }
}

// ---- the edge certificate (lrg_baseline_certify) ----
#define BL_EPS 2.220446049250313e-16
enum { BL_CERT_FALSE = 0, BL_CERT_TRUE = 1, BL_UNCERTAIN = 2 };

// The device's normals lie within s_i, s_k (per component) of LAPACK's, components in [0, 1]: the dot products differ by at most
// sqrt 3 (s_i + s_k) + 3 s_i s_k plus the FMA chain's own rounding, below E_n = 2 (s_i + s_k) + 3 s_i s_k + 8 eps.  The outcome
// d > t is certain when d is further than 2 E_n from t: one E_n for the solver, one for an edge whose other end has been replaced by
// LAPACK's value since.  Infinite slack or a NaN anywhere fails the comparison: uncertain.
__device__ __forceinline__ int bl_normal_conjunct(const BlArgs &a, int i, int k, double t) {
    const double d = bl_normal_dot(a.normals, i, k), si = a.nslack[i], sk = a.nslack[k];
    const double e = __dadd_rn(__dadd_rn(__dmul_rn(2.0, __dadd_rn(si, sk)), __dmul_rn(__dmul_rn(3.0, si), sk)), 8.0 * BL_EPS);
    if (!(fabs(__dsub_rn(d, t)) > __dmul_rn(2.0, e))) return BL_UNCERTAIN;
    return d > t ? BL_CERT_TRUE : BL_CERT_FALSE;
}

// | |c_k - c_i| - t | > 2 E_c, E_c = sc_i + sc_k + 2 eps
__device__ __forceinline__ int bl_curv_conjunct(const BlArgs &a, int i, int k, double t) {
    const double v = bl_curv_diff(a.curv, i, k);
    const double e = __dadd_rn(__dadd_rn(a.cslack[i], a.cslack[k]), 2.0 * BL_EPS);
    if (!(fabs(__dsub_rn(v, t)) > __dmul_rn(2.0, e))) return BL_UNCERTAIN;
    return v < t ? BL_CERT_TRUE : BL_CERT_FALSE;
}

// could the edge (i, k) come out differently under LAPACK?  At least one conjunct uncertain and none certainly false.
__device__ __forceinline__ bool bl_edge_uncertain(const BlArgs &a, int i, int k) {
    switch (a.mode) {
    case BL_NORMAL: case BL_SMOOTHNESS: return bl_normal_conjunct(a, i, k, a.t1) == BL_UNCERTAIN;
    case BL_CURVATURE: return bl_curv_conjunct(a, i, k, a.t1) == BL_UNCERTAIN;
    default: {                                                 // BL_FEATURE; the colour conjunct is float32 arithmetic on the raw data: certain
        const int cn = bl_normal_conjunct(a, i, k, a.t1), cc = bl_curv_conjunct(a, i, k, a.t2);
        if (cn == BL_CERT_FALSE || cc == BL_CERT_FALSE || !bl_color_edge(a.pts, a.ld, i, k, (float)a.t3)) return false;
        return cn == BL_UNCERTAIN || cc == BL_UNCERTAIN;
    }
    }
}

// the walk of bl_union_kernel; both ends of an uncertain edge get a 1 (every writer of a word writes the same value)
__global__ __launch_bounds__(BL_THREADS) void bl_certify_kernel(BlArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int r = a.room_of[i];
    if (r < 0) return;
    int s, e;
    if (!lrg_room_bounds(a.room_start, a.n, r, &s, &e)) return;
    uint64_t *keys; int32_t *vals; int mask;
    lrg_room_segment(a.keys, a.vals, r, s, e, &keys, &vals, &mask);
    const float *p = a.pts + (long)i * a.ld;
    const int vx = lrg_voxel_of(p[0], a.res), vy = lrg_voxel_of(p[1], a.res), vz = lrg_voxel_of(p[2], a.res);
    for (int dx = -1; dx <= 1; ++dx)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dz = -1; dz <= 1; ++dz) {
                if (!dx && !dy && !dz) continue;
                const int k = lrg_hash_lookup(keys, vals, mask, lrg_pack_voxel(vx + dx, vy + dy, vz + dz));
                if (k < 0 || k >= i) continue;
                if (bl_edge_uncertain(a, i, k)) { a.cflags[i] = 1; a.cflags[k] = 1; }
            }
}

// n_flagged = the number of flagged points (the flags are final: a launch boundary lies between)
__global__ __launch_bounds__(BL_THREADS) void bl_tally_kernel(BlArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int f = i < a.n ? a.cflags[i] != 0 : 0;
    const int c = __popcll(__ballot(f));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(a.n_flagged, c);
}

// One lane per covariance: prep_jacobi3, the selection of prep_eig_point, and how far LAPACK's values can lie from these.
__global__ __launch_bounds__(BL_THREADS) void bl_eig_kernel(const double *cov, int n, double *normals, double *curv, double *nslack,
                                                            double *cslack) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    double C[9], w[3], V[3][3];
    for (int k = 0; k < 9; ++k) C[k] = cov[(long)e * 9 + k];
    prep_jacobi3(C, w, V);
    const double s[3] = {fabs(w[0]), fabs(w[1]), fabs(w[2])};
    int i0, i1, i2;
    prep_eig_order(s, &i0, &i1, &i2);
    for (int k = 0; k < 3; ++k) normals[(long)e * 3 + k] = fabs(V[i2][k]);
    const double cv = fabs(s[i2] / (s[i0] + s[i1] + s[i2]));
    curv[e] = cv;
    // the vector of the smallest singular value moves by the perturbation over the gap to the next one; a (near-)degenerate pair or
    // a NaN curvature has no bound
    const double gap = s[i1] - s[i2];
    const bool bounded = gap > 1e-6 * s[i0] && cv == cv;
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    nslack[e] = bounded ? PREP_EIG_SLACK * s[i0] / gap : inf;
    cslack[e] = bounded ? PREP_EIG_SLACK : inf;
}

// every point's root (written back: the parents are final after the union launch), sizes, smoothness keys
__global__ __launch_bounds__(BL_THREADS) void bl_count_kernel(BlArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n || a.room_of[i] < 0) return;
    const int root = bl_find(a.parent, i);
    __hip_atomic_store(a.parent + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // every parent is its root after this launch
    atomicAdd(&a.size[root], 1);
    if (a.mode == BL_SMOOTHNESS) {
        const int s = a.room_start[a.room_of[i]], rk = a.rank[i];
        if (rk < 0 || rk >= a.room_start[a.room_of[i] + 1] - s) { atomicOr(&a.scal[0], BL_ST_RANK); return; }
        atomicMin(&a.minkey[root], ((unsigned long long)(unsigned)rk << 32) | (unsigned)(i - s));
    }
}

// The reference's DFS (:384-405) from `seed`: LIFO stack, neighbours pushed in offset order when unvisited and on an edge,
// visited marked at pop time.  Returns the pop count len(C), or -1 when the stack would overflow its reservation.
__device__ int bl_replay(const BlArgs &a, int s, int e, int r, int seed, int32_t *stk, int cap) {
    uint64_t *keys; int32_t *vals; int mask;
    lrg_room_segment(a.keys, a.vals, r, s, e, &keys, &vals, &mask);
    int top = 0, pops = 0;
    stk[top++] = seed;
    while (top > 0) {
        const int i = stk[--top];
        ++pops;
        a.visited[i] = 1;
        const float *p = a.pts + (long)i * a.ld;
        const int vx = lrg_voxel_of(p[0], a.res), vy = lrg_voxel_of(p[1], a.res), vz = lrg_voxel_of(p[2], a.res);
        for (int dx = -1; dx <= 1; ++dx)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dz = -1; dz <= 1; ++dz) {
                    if (!dx && !dy && !dz) continue;
                    const int k = lrg_hash_lookup(keys, vals, mask, lrg_pack_voxel(vx + dx, vy + dy, vz + dz));
                    if (k < 0 || a.visited[k] || !bl_normal_edge(a.normals, i, k, a.t1)) continue;
                    if (top >= cap) return -1;
                    stk[top++] = k;
                }
    }
    return pops;
}

__global__ __launch_bounds__(BL_THREADS) void bl_keep_kernel(BlArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int r = a.room_of[i];
    if (r < 0 || a.parent[i] != i) return;                  // one lane per component: its root
    const int s = a.room_start[r], e = a.room_start[r + 1], c = a.size[i];
    int key = i - s;
    bool keep = c > a.mcs;
    if (a.mode == BL_SMOOTHNESS) {
        const unsigned long long mk = a.minkey[i];
        if (mk == ~0ULL) return;                            // a rank was out of range (status set)
        key = (int)(mk >> 32);
        if (!keep && c >= 2) {
            const int cap = 1 + 26 * c;
            const long at = atomicAdd(&a.scal[1], cap);
            if (at + cap > a.stack_cap) { atomicOr(&a.scal[0], BL_ST_STACK); return; }
            const int pops = bl_replay(a, s, e, r, s + (int)(mk & 0xffffffffu), a.stack + at, cap);
            if (pops < 0) { atomicOr(&a.scal[0], BL_ST_STACK); return; }
            keep = pops > a.mcs;
        }
    }
    a.ckey[i] = key;
    if (keep) a.flag[s + key] = 1;
}

__global__ __launch_bounds__(BL_THREADS) void bl_label_kernel(BlArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.n_rooms) {
        int s, e;
        a.n_clusters[i] = lrg_room_bounds(a.room_start, a.n, i, &s, &e) ? a.scan[e] - a.scan[s] : 0;
    }
    if (i >= a.n) return;
    const int r = a.room_of[i];
    int lab = 0;
    if (r >= 0) {
        const int s = a.room_start[r], k = a.ckey[a.parent[i]];
        if (k >= 0 && a.flag[s + k]) lab = a.scan[s + k] - a.scan[s] + 1;
    }
    a.labels[i] = lab;
}

extern "C" {

size_t lrg_baseline_workspace_bytes(int n_points, int n_rooms, int min_cluster_size) {
    LrgBaselineLayout L;
    if (bl_layout(n_points, n_rooms, min_cluster_size, &L)) return 0;
    return L.total;
}

}  // extern "C"

// The checks and the argument block that lrg_baseline_segment, lrg_baseline_segment_embedding and lrg_baseline_certify share
// (room_start is copied to the workspace on the stream)
static int bl_setup(const float *pts, int ld, const int32_t *room_start, int n_rooms, float resolution, int mode, const double *normals,
                    const double *curvatures, const int32_t *rank, const float *emb, int dim, const int32_t *cls, double t1, double t2, double t3,
                    int min_cluster_size, void *ws, size_t ws_bytes, bool need_rank, bool have_outputs, hipStream_t st, LrgBaselineLayout *Lout, BlArgs *out) {
    LrgBaselineLayout &L = *Lout;
    if (n_rooms < 1 || n_rooms > (1 << 20) || !room_start || room_start[0] != 0) return LRG_EINVAL - 73;
    for (int r = 0; r < n_rooms; ++r)
        if (room_start[r + 1] < room_start[r]) return LRG_EINVAL - 73;
    const int n_points = room_start[n_rooms];
    int rc = bl_layout(n_points, n_rooms, min_cluster_size, &L);
    if (rc) return rc;
    if (mode < BL_NORMAL || mode > BL_MASK) return LRG_EINVAL - 72;
    if (mode == BL_EMBEDDING && (!emb || dim < 1 || dim > 64)) return LRG_EINVAL - 74;
    if (mode == BL_FPFH && (dim != BL_FPFH_DIM || (!emb && n_points > 0))) return LRG_EINVAL - 74;
    if (mode == BL_LABELS && !cls && n_points > 0) return LRG_EINVAL - 74;
    if (!ws || !have_outputs) return LRG_EINVAL - 73;
    if (n_points > 0 && (!pts || ld < 6)) return LRG_EINVAL - 73;
    const bool need_n = mode == BL_NORMAL || mode == BL_FEATURE || mode == BL_SMOOTHNESS;
    const bool need_c = mode == BL_CURVATURE || mode == BL_FEATURE;
    if ((need_n && !normals) || (need_c && !curvatures) || (need_rank && mode == BL_SMOOTHNESS && !rank)) return LRG_EINVAL - 74;
    if (ws_bytes < L.total || ((uintptr_t)ws & 255)) return LRG_EINVAL - 75;
    if (!(resolution > 0.f)) return LRG_EINVAL - 76;
    char *w = static_cast<char *>(ws);
    BlArgs a;
    int32_t *rooms = reinterpret_cast<int32_t *>(w + L.rooms);     // a device copy of room_start (the caller's is host memory)
    LRG_HIP_CHECK(hipMemcpyAsync(rooms, room_start, (size_t)(n_rooms + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
    a.pts = pts; a.ld = ld; a.room_start = rooms; a.n_rooms = n_rooms; a.n = n_points; a.res = resolution; a.mode = mode;
    a.normals = normals; a.curv = curvatures; a.rank = rank; a.emb = emb; a.dim = dim; a.cls = cls; a.keep = nullptr; a.unit = nullptr; a.t1 = t1; a.t2 = t2; a.t3 = t3; a.mcs = min_cluster_size;
    a.keys = reinterpret_cast<uint64_t *>(w + L.keys); a.vals = reinterpret_cast<int32_t *>(w + L.vals);
    a.room_of = reinterpret_cast<int32_t *>(w + L.room_of); a.parent = reinterpret_cast<int32_t *>(w + L.parent);
    a.size = reinterpret_cast<int32_t *>(w + L.size); a.minkey = reinterpret_cast<unsigned long long *>(w + L.minkey);
    a.ckey = reinterpret_cast<int32_t *>(w + L.ckey); a.visited = reinterpret_cast<int32_t *>(w + L.visited);
    a.flag = reinterpret_cast<int32_t *>(w + L.flag); a.scan = reinterpret_cast<int32_t *>(w + L.scan);
    a.bsum = reinterpret_cast<int32_t *>(w + L.bsum); a.stack = reinterpret_cast<int32_t *>(w + L.stack);
    a.scal = reinterpret_cast<int32_t *>(w + L.scal); a.hslots = L.hslots; a.stack_cap = L.stack_cap;
    a.labels = nullptr; a.n_clusters = nullptr;
    a.nslack = nullptr; a.cslack = nullptr; a.cflags = nullptr; a.n_flagged = nullptr;
    *out = a;
    return 0;
}

static inline int bl_init_grid(const LrgBaselineLayout &L, int n_points) {
    const long init_n = L.hslots > (long)n_points + 64 ? L.hslots : (long)n_points + 64;
    return (int)((init_n + BL_THREADS - 1) / BL_THREADS);
}

static inline size_t bl_fpfh_unit_bytes(int n_points) { return lrg_align_up((size_t)n_points * BL_FPFH_DIM * sizeof(double), 256); }

// lrg_baseline_segment and lrg_baseline_segment_embedding: the same checks and the same nine launches
static int bl_segment_impl(const float *pts, int ld, const int32_t *room_start, int n_rooms, float resolution, int mode,
                           const double *normals, const double *curvatures, const int32_t *rank, const float *emb, int dim, const int32_t *cls, double t1,
                           double t2, double t3, int min_cluster_size, void *ws, size_t ws_bytes, int32_t *labels, int32_t *n_clusters,
                           void *stream, const uint32_t *keep = nullptr) {
    LrgBaselineLayout L;
    BlArgs a;
    hipStream_t st = (hipStream_t)stream;
    if (mode == BL_MASK && !keep && room_start && n_rooms >= 1 && room_start[n_rooms] > 0) return LRG_EINVAL - 74;
    int rc = bl_setup(pts, ld, room_start, n_rooms, resolution, mode, normals, curvatures, rank, emb, dim, cls, t1, t2, t3, min_cluster_size, ws,
                      ws_bytes, true, labels && n_clusters, st, &L, &a);
    if (rc) return rc;
    const int n_points = a.n;
    a.labels = labels; a.n_clusters = n_clusters; a.keep = keep;
    if (mode == BL_FPFH) {                                     // the normalised histograms, behind the siblings' workspace
        if (ws_bytes < L.total + bl_fpfh_unit_bytes(n_points)) return LRG_EINVAL - 75;
        a.unit = reinterpret_cast<double *>(static_cast<char *>(ws) + L.total);
        if (n_points > 0)
            hipLaunchKernelGGL(bl_fpfh_unit_kernel, dim3((n_points + BL_THREADS - 1) / BL_THREADS), dim3(BL_THREADS), 0, st, emb, n_points, a.unit);
    }
    const int gi = bl_init_grid(L, n_points);
    const int gn = (int)(((long)(n_points > n_rooms ? n_points : n_rooms) + BL_THREADS - 1) / BL_THREADS);
    hipLaunchKernelGGL(bl_init_kernel, dim3(gi), dim3(BL_THREADS), 0, st, a);
    if (n_points > 0) {
        hipLaunchKernelGGL(bl_insert_kernel, dim3(gn), dim3(BL_THREADS), 0, st, a);
        hipLaunchKernelGGL(bl_union_kernel, dim3(gn), dim3(BL_THREADS), 0, st, a);
        hipLaunchKernelGGL(bl_count_kernel, dim3(gn), dim3(BL_THREADS), 0, st, a);
        hipLaunchKernelGGL(bl_keep_kernel, dim3(gn), dim3(BL_THREADS), 0, st, a);
    }
    if ((rc = lrg_exscan_i32(a.flag, (long)n_points + 1, a.bsum, a.scan, st))) return rc;      // flag[0 .. n] (n + 1 entries) into scan
    hipLaunchKernelGGL(bl_label_kernel, dim3(gn), dim3(BL_THREADS), 0, st, a);
    LRG_LAUNCH_CHECK();
    return 0;
}

extern "C" {

int lrg_baseline_segment(const float *pts, int ld, const int32_t *room_start, int n_rooms, float resolution, int mode,
                         const double *normals, const double *curvatures, const int32_t *rank, double t1, double t2, double t3,
                         int min_cluster_size, void *ws, size_t ws_bytes, int32_t *labels, int32_t *n_clusters, void *stream) {
    return bl_segment_impl(pts, ld, room_start, n_rooms, resolution, mode >= BL_EMBEDDING ? -1 : mode, normals, curvatures, rank, nullptr, 0, nullptr, t1, t2, t3,
                           min_cluster_size, ws, ws_bytes, labels, n_clusters, stream);
}

int lrg_baseline_segment_embedding(const float *pts, int ld, const int32_t *room_start, int n_rooms, float resolution, const float *emb,
                                   int dim, double t, int min_cluster_size, void *ws, size_t ws_bytes, int32_t *labels,
                                   int32_t *n_clusters, void *stream) {
    return bl_segment_impl(pts, ld, room_start, n_rooms, resolution, BL_EMBEDDING, nullptr, nullptr, nullptr, emb, dim, nullptr, t, 0.0, 0.0,
                           min_cluster_size, ws, ws_bytes, labels, n_clusters, stream);
}

int lrg_baseline_segment_labels(const float *pts, int ld, const int32_t *room_start, int n_rooms, float resolution, const int32_t *cls,
                                int min_cluster_size, void *ws, size_t ws_bytes, int32_t *labels, int32_t *n_clusters, void *stream) {
    return bl_segment_impl(pts, ld, room_start, n_rooms, resolution, BL_LABELS, nullptr, nullptr, nullptr, nullptr, 0, cls, 0.0, 0.0, 0.0,
                           min_cluster_size, ws, ws_bytes, labels, n_clusters, stream);
}

int lrg_baseline_segment_mask(const float *pts, int ld, const int32_t *room_start, int n_rooms, float resolution, const uint32_t *keep,
                              int min_cluster_size, void *ws, size_t ws_bytes, int32_t *labels, int32_t *n_clusters, void *stream) {
    return bl_segment_impl(pts, ld, room_start, n_rooms, resolution, BL_MASK, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0.0, 0.0, 0.0,
                           min_cluster_size, ws, ws_bytes, labels, n_clusters, stream, keep);
}

size_t lrg_baseline_fpfh_workspace_bytes(int n_points, int n_rooms, int min_cluster_size) {
    LrgBaselineLayout L;
    if (bl_layout(n_points, n_rooms, min_cluster_size, &L)) return 0;
    return L.total + bl_fpfh_unit_bytes(n_points);
}

int lrg_baseline_segment_fpfh(const float *pts, int ld, const int32_t *room_start, int n_rooms, float resolution, const float *hist, double t,
                              int min_cluster_size, void *ws, size_t ws_bytes, int32_t *labels, int32_t *n_clusters, void *stream) {
    return bl_segment_impl(pts, ld, room_start, n_rooms, resolution, BL_FPFH, nullptr, nullptr, nullptr, hist, BL_FPFH_DIM, nullptr, t, 0.0, 0.0,
                           min_cluster_size, ws, ws_bytes, labels, n_clusters, stream);
}

int lrg_baseline_eig(const double *cov, int n, double *normals, double *curvatures, double *normal_slack, double *curv_slack, void *stream) {
    if (n < 0 || n > (1 << 26)) return LRG_EINVAL - 77;
    if (n == 0) return 0;
    if (!cov || !normals || !curvatures || !normal_slack || !curv_slack) return LRG_EINVAL - 77;
    hipLaunchKernelGGL(bl_eig_kernel, dim3((n + BL_THREADS - 1) / BL_THREADS), dim3(BL_THREADS), 0, (hipStream_t)stream, cov, n, normals,
                       curvatures, normal_slack, curv_slack);
    LRG_LAUNCH_CHECK();
    return 0;
}

int lrg_baseline_certify(const float *pts, int ld, const int32_t *room_start, int n_rooms, float resolution, int mode, const double *normals,
                         const double *curvatures, const double *normal_slack, const double *curv_slack, double t1, double t2, double t3,
                         int min_cluster_size, void *ws, size_t ws_bytes, int32_t *flags, int32_t *n_flagged, void *stream) {
    LrgBaselineLayout L;
    BlArgs a;
    hipStream_t st = (hipStream_t)stream;
    if (mode >= BL_EMBEDDING) return LRG_EINVAL - 72;
    int rc = bl_setup(pts, ld, room_start, n_rooms, resolution, mode, normals, curvatures, nullptr, nullptr, 0, nullptr, t1, t2, t3, min_cluster_size,
                      ws, ws_bytes, false, flags && n_flagged, st, &L, &a);
    if (rc) return rc;
    const int n_points = a.n;
    if (mode == BL_COLOR) {                                        // float32 arithmetic on the raw data: nothing to certify, nothing launched
        if (n_points > 0) LRG_HIP_CHECK(hipMemsetAsync(flags, 0, (size_t)n_points * sizeof(int32_t), st));
        LRG_HIP_CHECK(hipMemsetAsync(n_flagged, 0, sizeof(int32_t), st));
        LRG_HIP_CHECK(hipMemsetAsync(a.scal, 0, sizeof(int32_t), st));
        return 0;
    }
    const bool need_n = mode != BL_CURVATURE, need_c = mode == BL_CURVATURE || mode == BL_FEATURE;
    if ((need_n && !normal_slack) || (need_c && !curv_slack)) return LRG_EINVAL - 74;
    a.nslack = normal_slack; a.cslack = curv_slack; a.cflags = flags; a.n_flagged = n_flagged;
    const int gn = (n_points + BL_THREADS - 1) / BL_THREADS;
    hipLaunchKernelGGL(bl_init_kernel, dim3(bl_init_grid(L, n_points)), dim3(BL_THREADS), 0, st, a);
    if (n_points > 0) {
        hipLaunchKernelGGL(bl_insert_kernel, dim3(gn), dim3(BL_THREADS), 0, st, a);
        hipLaunchKernelGGL(bl_certify_kernel, dim3(gn), dim3(BL_THREADS), 0, st, a);
        hipLaunchKernelGGL(bl_tally_kernel, dim3(gn), dim3(BL_THREADS), 0, st, a);
    }
    LRG_LAUNCH_CHECK();
    return 0;
}

int lrg_baseline_status(const void *ws, int n_points, int n_rooms, int min_cluster_size, int32_t *host_status, void *stream) {
    LrgBaselineLayout L;
    int rc = bl_layout(n_points, n_rooms, min_cluster_size, &L);
    if (rc) return rc;
    if (!ws || !host_status) return LRG_EINVAL - 73;
    LRG_HIP_CHECK(hipMemcpyAsync(host_status, static_cast<const char *>(ws) + L.scal, sizeof(int32_t), hipMemcpyDeviceToHost,
                                 (hipStream_t)stream));
    LRG_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

}  // extern "C"
