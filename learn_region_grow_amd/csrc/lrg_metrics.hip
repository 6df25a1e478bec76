// Per-room evaluation metrics of all rooms of a call in one pass (test_region_grow.py:319-355, test_mcpnet.py:146-170): contingency
// tables, the integer sums of the adjusted Rand score, entropies / mutual information / expected mutual information with sklearn's
// arithmetic, the greedy IoU > 0.5 matching and the relabelled clusters.  The rooms' points lie one after the other; every kernel
// runs over all rooms (flat over points, cells or chunks, or one workgroup per room), so the launch count does not depend on the
// number of rooms.  Determinism: integer atomics only (their sums do not depend on arrival order); every float64 sum is written as
// partials whose bounds depend on the room alone and added by one workgroup per room in a fixed order -- a room's outputs in a batch
// are the bits of that room in a batch of its own.
#include "lrg_common.h"

#define MT_THREADS 256
#define MT_TILE 2048            // points per workgroup of the contingency kernel
#define MT_LDS_CELLS 8192       // a table of up to this many int32 cells (32 KB) is privatised in LDS; larger ones take global atomics
#define MT_CHUNK 32             // EMI terms per chunk: one thread sums one chunk, no thread owns a whole (i, j) pair
#define MT_MAX_ROOMS 65536
#define MT_ROOM_CELLS (1L << 24)   // table cells of one room (its scans are one workgroup's)
#define MT_ISUMS 8              // per room int64: sum nij^2, sum a^2, sum b^2, N counted, non-empty rows, non-empty columns, EMI terms, EMI chunks
#define MT_FSUMS 4              // per room float64: H(true), H(pred), MI (unclipped), EMI

struct MtLayout {
    size_t room_start, gt_start, ncl, col_start, cell_start, chunk_base, status;      // per room
    size_t cont, cchunk, a, b, map, T, partial;
    size_t total;
    long n, g, cols, cells, chunks;
    int max_n;
};

struct MtArgs {
    const int32_t *labels, *gt_row, *order, *relabel, *unmatched_base;
    int32_t *room_start, *gt_start, *ncl, *col_start, *cell_start, *chunk_base, *status;
    int n_rooms, n, max_n, scores;
    long g, cols, cells, chunks;
    int32_t *cont, *cchunk, *a, *b, *map;
    double *T, *partial;
    int32_t *label2; double *best_iou; uint8_t *dt_match; int32_t *gt_match; long long *isums; double *fsums;
};

// upper bound of a room's EMI chunks: every non-empty pair has ceil(L / MT_CHUNK) <= 1 + L / MT_CHUNK of them, and the lengths L <= min(a_i, b_j)
// sum to at most min(G, C + 1) N
static __host__ __device__ inline long mt_chunk_bound(long n, long g, long w) {
    return g * w + ((g < w ? g : w) * n) / MT_CHUNK + 1;
}

// the starts are host memory: checked here, before anything is launched
static int mt_layout(const int32_t *room_start, const int32_t *gt_start, const int32_t *n_cluster, int n_rooms, MtLayout *L) {
    if (n_rooms < 1 || n_rooms > MT_MAX_ROOMS || !room_start || !gt_start || !n_cluster || room_start[0] != 0 || gt_start[0] != 0)
        return LRG_EINVAL - 90;
    for (int r = 0; r < n_rooms; ++r) {
        if (room_start[r + 1] < room_start[r] || gt_start[r + 1] < gt_start[r]) return LRG_EINVAL - 91;
        if (room_start[r + 1] == room_start[r] || gt_start[r + 1] == gt_start[r]) return LRG_EINVAL - 92;     // an empty room, or one without a GT row
        if (n_cluster[r] < 0) return LRG_EINVAL - 93;
    }
    const long n = room_start[n_rooms], g = gt_start[n_rooms];
    if (n >= (1L << 30) || g >= (1L << 30)) return LRG_EINVAL - 94;
    long cols = 0, cells = 0, chunks = 0;
    int max_n = 0;
    for (int r = 0; r < n_rooms; ++r) {
        const long nr = room_start[r + 1] - room_start[r], gr = gt_start[r + 1] - gt_start[r], w = (long)n_cluster[r] + 1;
        if (gr * w > MT_ROOM_CELLS) return LRG_EINVAL - 94;
        cols += w; cells += gr * w; chunks += mt_chunk_bound(nr, gr, w);
        if (cols >= (1L << 30) || cells >= (1L << 30) || chunks >= (1L << 31) - MT_THREADS) return LRG_EINVAL - 94;
        if (nr > max_n) max_n = (int)nr;
    }
    L->n = n; L->g = g; L->cols = cols; L->cells = cells; L->chunks = chunks; L->max_n = max_n;
    LrgArena ws;
    L->room_start = ws.take((size_t)(n_rooms + 1) * 4);
    L->gt_start = ws.take((size_t)(n_rooms + 1) * 4);
    L->ncl = ws.take((size_t)n_rooms * 4);
    L->col_start = ws.take((size_t)(n_rooms + 1) * 4);
    L->cell_start = ws.take((size_t)(n_rooms + 1) * 4);
    L->chunk_base = ws.take((size_t)(n_rooms + 1) * 4);
    L->status = ws.take((size_t)n_rooms * 4);
    L->cont = ws.take((size_t)cells * 4);
    L->cchunk = ws.take((size_t)cells * 4);
    L->a = ws.take((size_t)g * 4);
    L->b = ws.take((size_t)cols * 4);
    L->map = ws.take((size_t)cols * 4);
    L->T = ws.take((size_t)(max_n + 1) * 8);
    L->partial = ws.take((size_t)chunks * 8);
    L->total = ws.total;
    return 0;
}

// fixed-order sum of one value per thread (MT_THREADS threads); the result is returned to every thread
__device__ __forceinline__ double mt_block_sum(double v, double *s_red) {
    __syncthreads();
    s_red[threadIdx.x] = v;
    __syncthreads();
    for (int s = MT_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) s_red[threadIdx.x] += s_red[threadIdx.x + s];
        __syncthreads();
    }
    return s_red[0];
}

__device__ __forceinline__ long long mt_block_sum_i64(long long v, long long *s_red) {
    __syncthreads();
    s_red[threadIdx.x] = v;
    __syncthreads();
    for (int s = MT_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) s_red[threadIdx.x] += s_red[threadIdx.x + s];
        __syncthreads();
    }
    return s_red[0];
}

// one workgroup: the rooms' column / cell / chunk starts from the copied host arrays, and the per-room outputs zeroed
__global__ __launch_bounds__(MT_THREADS) void mt_layout_kernel(MtArgs a) {
    if (threadIdx.x == 0) {
        long cols = 0, cells = 0, chunks = 0;
        for (int r = 0; r < a.n_rooms; ++r) {
            a.col_start[r] = (int32_t)cols; a.cell_start[r] = (int32_t)cells; a.chunk_base[r] = (int32_t)chunks;
            const long nr = a.room_start[r + 1] - a.room_start[r], gr = a.gt_start[r + 1] - a.gt_start[r], w = (long)a.ncl[r] + 1;
            cols += w; cells += gr * w; chunks += mt_chunk_bound(nr, gr, w);
        }
        a.col_start[a.n_rooms] = (int32_t)cols; a.cell_start[a.n_rooms] = (int32_t)cells; a.chunk_base[a.n_rooms] = (int32_t)chunks;
    }
    for (int r = threadIdx.x; r < a.n_rooms; r += MT_THREADS) {
        a.status[r] = 0;
        a.gt_match[r] = 0;
        for (int k = 0; k < MT_ISUMS; ++k) a.isums[(long)r * MT_ISUMS + k] = 0;
        for (int k = 0; k < MT_FSUMS; ++k) a.fsums[(long)r * MT_FSUMS + k] = 0.0;
    }
}

__global__ __launch_bounds__(MT_THREADS) void mt_init_kernel(MtArgs a) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < a.cells; t += stride) a.cont[t] = 0;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < a.g; t += stride) a.a[t] = 0;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < a.cols; t += stride) { a.b[t] = 0; a.map[t] = 0; }
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < a.cols - a.n_rooms; t += stride) a.dt_match[t] = 0;
}

// T[k] = lgamma(k + 1), one table for all rooms
__global__ __launch_bounds__(MT_THREADS) void mt_lgamma_table_kernel(double *T, int max_n) {
    const long k = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k <= max_n) T[k] = lgamma((double)k + 1.0);
}

// cont[g, j] of every room.  A workgroup owns MT_TILE consecutive points; when they belong to one room whose table fits MT_LDS_CELLS the
// counts are gathered in LDS first and the non-zero cells added to the room's table, otherwise every point adds to global memory.
__global__ __launch_bounds__(MT_THREADS) void mt_cont_kernel(MtArgs a) {
    __shared__ int32_t s_tab[MT_LDS_CELLS];
    const long first = (long)blockIdx.x * MT_TILE;
    if (first >= a.n) return;
    const int lo = (int)first, hi = (int)(first + MT_TILE < (long)a.n ? first + MT_TILE : (long)a.n);
    const int r0 = lrg_last_start(a.room_start, 0, a.n_rooms - 1, lo), r1 = lrg_last_start(a.room_start, r0, a.n_rooms - 1, hi - 1);
    const int g0 = a.gt_start[r0 + 1] - a.gt_start[r0], w0 = a.ncl[r0] + 1;
    const bool lds = r0 == r1 && (long)g0 * w0 <= MT_LDS_CELLS;
    if (lds) {
        const int cells = g0 * w0;
        for (int c = threadIdx.x; c < cells; c += MT_THREADS) s_tab[c] = 0;
        __syncthreads();
        for (int i = lo + (int)threadIdx.x; i < hi; i += MT_THREADS) {
            const int lab = a.labels[i], g = a.gt_row[i];
            if ((unsigned)lab >= (unsigned)w0 || (unsigned)g >= (unsigned)g0) { atomicOr(&a.status[r0], 1); continue; }
            atomicAdd(&s_tab[g * w0 + lab], 1);
        }
        __syncthreads();
        int32_t *cont = a.cont + a.cell_start[r0];
        for (int c = threadIdx.x; c < cells; c += MT_THREADS) {
            const int v = s_tab[c];
            if (v) atomicAdd(&cont[c], v);
        }
    } else {
        for (int i = lo + (int)threadIdx.x; i < hi; i += MT_THREADS) {
            const int r = lrg_last_start(a.room_start, r0, r1, i);
            const int G = a.gt_start[r + 1] - a.gt_start[r], W = a.ncl[r] + 1;
            const int lab = a.labels[i], g = a.gt_row[i];
            if ((unsigned)lab >= (unsigned)W || (unsigned)g >= (unsigned)G) { atomicOr(&a.status[r], 1); continue; }
            atomicAdd(&a.cont[(long)a.cell_start[r] + (long)g * W + lab], 1);
        }
    }
}

// row sums a, column sums b and sum nij^2, flat over the cells of all rooms (integer atomics: the same bits in any order)
__global__ __launch_bounds__(MT_THREADS) void mt_sums_kernel(MtArgs a) {
    __shared__ long long s_red[MT_THREADS];
    const long first = (long)blockIdx.x * MT_THREADS;
    if (first >= a.cells) return;
    const long last = first + MT_THREADS - 1 < a.cells - 1 ? first + MT_THREADS - 1 : a.cells - 1;
    const int r0 = lrg_last_start(a.cell_start, 0, a.n_rooms - 1, (int)first), r1 = lrg_last_start(a.cell_start, r0, a.n_rooms - 1, (int)last);
    const long c = first + threadIdx.x;
    long long sq = 0;
    int r = r0;
    if (c < a.cells) {
        const int v = a.cont[c];
        if (v) {
            r = lrg_last_start(a.cell_start, r0, r1, (int)c);
            const int W = a.ncl[r] + 1, rel = (int)(c - a.cell_start[r]);
            atomicAdd(&a.a[a.gt_start[r] + rel / W], v);
            atomicAdd(&a.b[a.col_start[r] + rel % W], v);
            sq = (long long)v * v;
        }
    }
    if (r0 == r1) {                                  // (uniform: one room's cells, one add for the workgroup)
        const long long s = mt_block_sum_i64(sq, s_red);
        if (threadIdx.x == 0 && s) atomicAdd((unsigned long long *)&a.isums[(long)r0 * MT_ISUMS + 0], (unsigned long long)s);
    } else if (sq) {
        atomicAdd((unsigned long long *)&a.isums[(long)r * MT_ISUMS + 0], (unsigned long long)sq);
    }
}

// length of the nij range of sklearn's expected_mutual_information for a pair with row sum ai and column sum bj
__device__ __forceinline__ int mt_pair_len(int ai, int bj, int N, int *start) {
    if (ai <= 0 || bj <= 0) { *start = 1; return 0; }
    const int s = max(1, ai + bj - N), e = min(ai, bj);
    *start = s;
    return e >= s ? e - s + 1 : 0;
}

// One workgroup per room: counts of non-empty rows / columns, sum a^2, sum b^2, N; with scores the entropies and the mutual information
// (sklearn's entropy and mutual_info_score term by term; thread t adds the terms t, t + 256, ... and the 256 sums meet in a fixed tree)
// and the exclusive scan of the pairs' chunk counts.
__global__ __launch_bounds__(MT_THREADS) void mt_room_kernel(MtArgs a) {
    __shared__ double s_redf[MT_THREADS];
    __shared__ long long s_redi[MT_THREADS];
    __shared__ int s_wave[MT_THREADS / 64];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int G = a.gt_start[r + 1] - a.gt_start[r], W = a.ncl[r] + 1;
    const int32_t *ar = a.a + a.gt_start[r], *br = a.b + a.col_start[r];
    const int32_t *cont = a.cont + a.cell_start[r];
    long long *is = a.isums + (long)r * MT_ISUMS;
    double *fs = a.fsums + (long)r * MT_FSUMS;
    long long sa2 = 0, sb2 = 0, sn = 0, rows = 0, cols = 0;
    for (int g = tid; g < G; g += MT_THREADS) { const long long v = ar[g]; sa2 += v * v; sn += v; rows += v > 0; }
    for (int j = tid; j < W; j += MT_THREADS) { const long long v = br[j]; sb2 += v * v; cols += v > 0; }
    sa2 = mt_block_sum_i64(sa2, s_redi);
    sb2 = mt_block_sum_i64(sb2, s_redi);
    sn = mt_block_sum_i64(sn, s_redi);
    rows = mt_block_sum_i64(rows, s_redi);
    cols = mt_block_sum_i64(cols, s_redi);
    if (tid == 0) { is[1] = sa2; is[2] = sb2; is[3] = sn; is[4] = rows; is[5] = cols; }
    if (!a.scores || sn <= 0) return;
    const int N = (int)sn;
    const double dN = (double)N, logN = log(dN);
    // entropies: -sum (p / N) (log p - log N)
    double h = 0.0;
    for (int g = tid; g < G; g += MT_THREADS) { const int v = ar[g]; if (v > 0) h += ((double)v / dN) * (log((double)v) - logN); }
    h = mt_block_sum(h, s_redf);
    if (tid == 0) fs[0] = -h;
    h = 0.0;
    for (int j = tid; j < W; j += MT_THREADS) { const int v = br[j]; if (v > 0) h += ((double)v / dN) * (log((double)v) - logN); }
    h = mt_block_sum(h, s_redf);
    if (tid == 0) fs[1] = -h;
    // mutual information over the non-zero cells, and the chunk counts of all pairs (tiles of 256 cells in order)
    const int cells = G * W;
    int32_t *cchunk = a.cchunk + a.cell_start[r];
    double mi = 0.0;
    long long terms = 0;
    int carry = 0;
    for (int base = 0; base < cells; base += MT_THREADS) {
        const int c = base + tid;
        int nch = 0;
        if (c < cells) {
            const int g = c / W, j = c % W;
            const int ai = ar[g], bj = br[j], v = cont[c];
            if (v > 0) {
                const double nm = (double)v / dN;
                const double log_outer = -log((double)((long long)ai * (long long)bj)) + logN + logN;
                const double t = nm * (log((double)v) - logN) + nm * log_outer;
                mi += fabs(t) < 2.220446049250313e-16 ? 0.0 : t;
            }
            int start;
            const int len = mt_pair_len(ai, bj, N, &start);
            terms += len;
            nch = (len + MT_CHUNK - 1) / MT_CHUNK;
        }
        const int incl = lrg_wave_incl_scan_i32(nch);
        __syncthreads();
        if ((tid & 63) == 63) s_wave[tid >> 6] = incl;
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < MT_THREADS / 64; ++w) { const int v = s_wave[w]; if (w < (tid >> 6)) before += v; total += v; }
        if (c < cells) cchunk[c] = carry + before + incl - nch;
        carry += total;
    }
    mi = mt_block_sum(mi, s_redf);
    terms = mt_block_sum_i64(terms, s_redi);
    if (tid == 0) { fs[2] = mi; is[6] = terms; is[7] = carry; }
}

// Expected mutual information, sklearn's _expected_mutual_info_fast.pyx term by term: one thread per chunk of at most MT_CHUNK consecutive
// nij of one (i, j) pair.  Chunks are numbered room by room through the scan of mt_room_kernel; the partial of chunk q of room r lands at
// chunk_base[r] + q.  A term whose gln is below -746 has exp(gln) == 0 exactly and adds +-0: leaving it out changes no bit.
__global__ __launch_bounds__(MT_THREADS) void mt_emi_kernel(MtArgs a) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.chunks) return;
    const int r = lrg_last_start(a.chunk_base, 0, a.n_rooms - 1, (int)t);
    const int q = (int)(t - a.chunk_base[r]);
    const long long *is = a.isums + (long)r * MT_ISUMS;
    const long room_bound = (long)a.chunk_base[r + 1] - a.chunk_base[r];
    if (q >= is[7] || q >= room_bound) return;
    const int G = a.gt_start[r + 1] - a.gt_start[r], W = a.ncl[r] + 1, N = (int)is[3];
    const int32_t *cchunk = a.cchunk + a.cell_start[r];
    const int c = lrg_last_start(cchunk, 0, G * W - 1, q);
    const int ai = a.a[a.gt_start[r] + c / W], bj = a.b[a.col_start[r] + c % W];
    int start;
    const int len = mt_pair_len(ai, bj, N, &start);
    const int k = q - cchunk[c];
    const int s = start + k * MT_CHUNK;
    const int e = min(start + len - 1, s + MT_CHUNK - 1);
    const double *T = a.T;
    const double dN = (double)N, logN = log(dN), log_a = log((double)ai), log_b = log((double)bj);
    const double g4 = T[ai] + T[bj] + T[N - ai] + T[N - bj], TN = T[N];
    double emi = 0.0;
    for (int nij = s; nij <= e; ++nij) {
        const double gln = g4 - (T[nij] + TN) - T[ai - nij] - T[bj - nij] - T[N - ai - bj + nij];
        if (gln < -746.0) continue;
        const double term1 = (double)nij / dN;
        const double term2 = (logN + log((double)nij)) - log_a - log_b;
        const double term3 = exp(gln);
        emi += term1 * term2 * term3;
    }
    a.partial[t] = emi;
}

// one workgroup per room: the room's chunk partials in a fixed order
__global__ __launch_bounds__(MT_THREADS) void mt_emi_sum_kernel(MtArgs a) {
    __shared__ double s_redf[MT_THREADS];
    const int r = blockIdx.x;
    const long long *is = a.isums + (long)r * MT_ISUMS;
    const long bound = (long)a.chunk_base[r + 1] - a.chunk_base[r];
    const long n = is[7] < bound ? is[7] : bound;
    const double *p = a.partial + a.chunk_base[r];
    double s = 0.0;
    for (long q = threadIdx.x; q < n; q += MT_THREADS) s += p[q];
    s = mt_block_sum(s, s_redf);
    if (threadIdx.x == 0) a.fsums[(long)r * MT_FSUMS + 3] = s;
}

// Greedy matching, one workgroup per room (:327-341).  For a GT row g at most one still-unmatched cluster has iou > 0.5 (the clusters are
// disjoint and each such cluster holds more than half of g's points; the quotient of exact integers rounds monotonically, so the float64
// test is the exact one), and it is then the row's maximum: the first j with iou > 0.5 and the maximum over the unmatched j up to it are
// the minimum such j and the maximum over all unmatched j.  Maxima of non-negative doubles are taken on their bit patterns.
__global__ __launch_bounds__(MT_THREADS) void mt_match_kernel(MtArgs a) {
    __shared__ unsigned long long s_best;
    __shared__ int s_j;
    const int r = blockIdx.x, tid = threadIdx.x;
    const int G = a.gt_start[r + 1] - a.gt_start[r], W = a.ncl[r] + 1, C = W - 1;
    const int32_t *ar = a.a + a.gt_start[r], *br = a.b + a.col_start[r];
    const int32_t *cont = a.cont + a.cell_start[r];
    const int32_t *order = a.order + a.gt_start[r], *relabel = a.relabel + a.gt_start[r];
    uint8_t *dt = a.dt_match + (a.col_start[r] - r);
    int32_t *map = a.map + a.col_start[r];
    double *best = a.best_iou + a.gt_start[r];
    int matched = 0;
    for (int k = 0; k < G; ++k) {
        if (tid == 0) { s_best = 0ULL; s_j = INT_MAX; }
        __syncthreads();
        const int g = order[k];
        if ((unsigned)g < (unsigned)G) {
            const long long cg = ar[g];
            unsigned long long mx = 0ULL;
            int jm = INT_MAX;
            for (int j = tid + 1; j <= C; j += MT_THREADS) {
                if (dt[j - 1]) continue;
                const long long inter = cont[(long)g * W + j], den = cg + br[j] - inter;
                if (den <= 0) continue;
                const double iou = 1.0 * (double)inter / (double)den;
                const unsigned long long bits = (unsigned long long)__double_as_longlong(iou);
                if (bits > mx) mx = bits;
                if (iou > 0.5 && j < jm) jm = j;
            }
            if (mx) atomicMax(&s_best, mx);
            if (jm != INT_MAX) atomicMin(&s_j, jm);
        } else if (tid == 0) {
            atomicOr(&a.status[r], 2);
        }
        __syncthreads();
        if (tid == 0) {
            best[k] = __longlong_as_double((long long)s_best);
            if (s_j != INT_MAX) { dt[s_j - 1] = 1; map[s_j] = relabel[k]; ++matched; }
        }
        __syncthreads();
    }
    const int base = a.unmatched_base[r];
    for (int j = tid + 1; j <= C; j += MT_THREADS)
        if (!dt[j - 1]) map[j] = j + base;
    if (tid == 0) { map[0] = 0; a.gt_match[r] = matched; }
}

__global__ __launch_bounds__(MT_THREADS) void mt_relabel_kernel(MtArgs a) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.n) return;
    const int i = (int)t;
    const int r = lrg_last_start(a.room_start, 0, a.n_rooms - 1, i);
    const int lab = a.labels[i];
    a.label2[i] = (unsigned)lab <= (unsigned)a.ncl[r] ? a.map[a.col_start[r] + lab] : 0;
}

static MtArgs mt_carve(const MtLayout &L, void *workspace, int n_rooms) {
    char *ws = static_cast<char *>(workspace);
    auto i32 = [&](size_t at) { return reinterpret_cast<int32_t *>(ws + at); };
    MtArgs a = {};
    a.room_start = i32(L.room_start); a.gt_start = i32(L.gt_start); a.ncl = i32(L.ncl); a.col_start = i32(L.col_start);
    a.cell_start = i32(L.cell_start); a.chunk_base = i32(L.chunk_base); a.status = i32(L.status);
    a.n_rooms = n_rooms; a.n = (int)L.n; a.max_n = L.max_n; a.g = L.g; a.cols = L.cols; a.cells = L.cells; a.chunks = L.chunks;
    a.cont = i32(L.cont); a.cchunk = i32(L.cchunk); a.a = i32(L.a); a.b = i32(L.b); a.map = i32(L.map);
    a.T = reinterpret_cast<double *>(ws + L.T); a.partial = reinterpret_cast<double *>(ws + L.partial);
    return a;
}

extern "C" {

size_t lrg_metrics_batch_workspace_bytes(const int32_t *room_start, const int32_t *gt_start, const int32_t *n_cluster, int n_rooms) {
    MtLayout L;
    if (mt_layout(room_start, gt_start, n_cluster, n_rooms, &L) != 0) return 0;
    return L.total;
}

int lrg_metrics_batch(const int32_t *labels, const int32_t *gt_row, const int32_t *order, const int32_t *relabel, const int32_t *unmatched_base,
                      const int32_t *room_start, const int32_t *gt_start, const int32_t *n_cluster, int n_rooms, unsigned flags,
                      void *workspace, size_t workspace_bytes, int32_t *cluster_label2, double *best_iou, uint8_t *dt_match,
                      int32_t *gt_match, int64_t *int_sums, double *float_sums, void *stream) {
    MtLayout L;
    int rc = mt_layout(room_start, gt_start, n_cluster, n_rooms, &L);
    if (rc) return rc;
    if (!labels || !gt_row || !order || !relabel || !unmatched_base || !workspace || !cluster_label2 || !best_iou || !dt_match || !gt_match ||
        !int_sums || !float_sums)
        return LRG_EINVAL - 95;
    if (workspace_bytes < L.total || ((uintptr_t)workspace & 255)) return LRG_EINVAL - 96;
    hipStream_t st = (hipStream_t)stream;
    MtArgs a = mt_carve(L, workspace, n_rooms);
    // device copies of the three host arrays
    LRG_HIP_CHECK(hipMemcpyAsync(a.room_start, room_start, (size_t)(n_rooms + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
    LRG_HIP_CHECK(hipMemcpyAsync(a.gt_start, gt_start, (size_t)(n_rooms + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
    LRG_HIP_CHECK(hipMemcpyAsync(a.ncl, n_cluster, (size_t)n_rooms * sizeof(int32_t), hipMemcpyHostToDevice, st));
    a.labels = labels; a.gt_row = gt_row; a.order = order; a.relabel = relabel; a.unmatched_base = unmatched_base;
    a.scores = (flags & 1u) ? 0 : 1;
    a.label2 = cluster_label2; a.best_iou = best_iou; a.dt_match = dt_match; a.gt_match = gt_match;
    a.isums = reinterpret_cast<long long *>(int_sums); a.fsums = float_sums;
    auto blocks = [](long n) { return dim3((unsigned)((n + MT_THREADS - 1) / MT_THREADS)); };
    long most = L.cells > L.cols ? L.cells : L.cols;
    if (L.g > most) most = L.g;
    const long init_blocks = (most + MT_THREADS - 1) / MT_THREADS;
    hipLaunchKernelGGL(mt_layout_kernel, dim3(1), dim3(MT_THREADS), 0, st, a);
    hipLaunchKernelGGL(mt_init_kernel, dim3((unsigned)(init_blocks < 4096 ? init_blocks : 4096)), dim3(MT_THREADS), 0, st, a);
    if (a.scores) hipLaunchKernelGGL(mt_lgamma_table_kernel, blocks((long)L.max_n + 1), dim3(MT_THREADS), 0, st, a.T, L.max_n);
    hipLaunchKernelGGL(mt_cont_kernel, dim3((unsigned)((L.n + MT_TILE - 1) / MT_TILE)), dim3(MT_THREADS), 0, st, a);
    hipLaunchKernelGGL(mt_sums_kernel, blocks(L.cells), dim3(MT_THREADS), 0, st, a);
    hipLaunchKernelGGL(mt_room_kernel, dim3(n_rooms), dim3(MT_THREADS), 0, st, a);
    LRG_LAUNCH_CHECK();
    if (a.scores) {
        hipLaunchKernelGGL(mt_emi_kernel, blocks(L.chunks), dim3(MT_THREADS), 0, st, a);
        hipLaunchKernelGGL(mt_emi_sum_kernel, dim3(n_rooms), dim3(MT_THREADS), 0, st, a);
    }
    hipLaunchKernelGGL(mt_match_kernel, dim3(n_rooms), dim3(MT_THREADS), 0, st, a);
    hipLaunchKernelGGL(mt_relabel_kernel, blocks(L.n), dim3(MT_THREADS), 0, st, a);
    LRG_LAUNCH_CHECK();
    return 0;
}

/* per-room flags of the last lrg_metrics_batch on this workspace: 1 = a label or a GT row out of range (skipped), 2 = a bad `order` entry */
int lrg_metrics_batch_status(const void *workspace, const int32_t *room_start, const int32_t *gt_start, const int32_t *n_cluster, int n_rooms,
                             int32_t *host_status_per_room, void *stream) {
    MtLayout L;
    int rc = mt_layout(room_start, gt_start, n_cluster, n_rooms, &L);
    if (rc) return rc;
    if (!workspace || !host_status_per_room) return LRG_EINVAL - 95;
    LRG_HIP_CHECK(hipMemcpyAsync(host_status_per_room, static_cast<const char *>(workspace) + L.status, (size_t)n_rooms * sizeof(int32_t),
                                 hipMemcpyDeviceToHost, (hipStream_t)stream));
    LRG_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

}  // extern "C"
