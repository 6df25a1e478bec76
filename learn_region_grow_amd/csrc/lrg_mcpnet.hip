// MCPNet (test_mcpnet.py, learn_region_grow_util.py:191-225) for gfx950: candidate lists, neighbour draws and the embedding network.
//
// Candidates (test_mcpnet.py:75-107).  Every equalised point goes into the coarse cell round(x / 0.3) of its room; the candidates of
// point i are the members of the 27 cells around its own cell, cells in itertools.product(range(-1, 2), ...) order (dz fastest),
// members in ascending index, i itself included.  lrg_mcp_candidates builds a per-room cell table in a fixed sequence of launches:
//   init     hash slots empty, cell counts cleared, the room of every point (binary search in room_start)
//   insert   coarse key -> the room's own linear-probe segment; find-or-insert by CAS, then a count per cell
//   scan     exclusive scan of the cell counts (three launches): the start of each cell's member list
//   fill     every point at a free position of its cell's list
//   sort     one lane per cell: its members in ascending index (insertion sort; a cell holds at most a few dozen points)
//   count    the candidate count of every point
// lrg_mcp_neighbors then maps 50 positions per point into the candidate list to point indices: positions drawn on the host
// (legacy: numpy.random.choice in room order) or on the device (counter: Philox keyed by (seed, room id)).
//
// Embedding (lrg_mcp_embed).  One wavefront per 16 points = 800 rows = 25 row tiles of 32: the rows of a point never pad.
//   layer 1  each lane computes 100 columns of its row (lane half h: columns 2 s + h), relu, straight into A-operand registers
//   layer 2  v_mfma_f32_32x32x2_f32 over the 100 k-steps per 32-column tile (7 tiles, 224 >= 200 columns); the weights come
//            pre-arranged in operand order (lrg_mcp_pack_weights), one global_load_dwordx4 per lane per four k-steps, through a
//            ring five groups ahead
//   pool     bias, relu, the max of each lane's rows per point, then one LDS max per point and column (relu output >= +0, so the
//            float bits order as unsigned integers)
//   head     concat(z, r, g, b, pooled) -> 200 (relu) -> 10 in fp32 FMA chains, then x * (1 / sqrt(max(sum x^2, 1e-12)))
#include "lrg_common.h"
#include "lrg_rng.h"
#include "lrg_room_hash.h"

#define MCP_THREADS 256
#include "lrg_mcp_layout.h"
#define MCP_PTS 16                   // points per wavefront: 800 rows = 25 tiles of 32

// status bits (lrg_mcp_status)
enum { MCP_ST_WINDOW = 1, MCP_ST_POSITION = 2 };

struct LrgMcpLayout {
    size_t keys, cnt, off, fill, members, cell, room_of, rooms, rids, bsum, scal, total;
    long hslots;
};

static int mcp_layout(int N, int R, LrgMcpLayout *L) {
    if (N < 0 || R < 1 || N > (1 << 26) || R > (1 << 20)) return LRG_EINVAL - 80;
    L->hslots = lrg_room_hash_slots(N, R);
    LrgArena ws;
    L->keys = ws.take((size_t)L->hslots * 8);
    L->cnt = ws.take((size_t)(L->hslots + 1) * 4);
    L->off = ws.take((size_t)(L->hslots + 1) * 4);
    L->fill = ws.take((size_t)L->hslots * 4);
    L->members = ws.take((size_t)N * 4 + 4);
    L->cell = ws.take((size_t)N * 4 + 4);
    L->room_of = ws.take((size_t)N * 4 + 4);
    L->rooms = ws.take((size_t)(R + 1) * 4);
    L->rids = ws.take((size_t)R * 4);
    L->bsum = ws.take((size_t)(lrg_scan_blocks(L->hslots + 1) + 1) * 4);
    L->scal = ws.take(64 * 4);
    L->total = ws.total;
    return 0;
}

struct McpArgs {
    const float *pts; int ld;
    const int32_t *room_start, *rids; int n_rooms, n;
    uint64_t *keys; int32_t *cnt, *off, *fill, *members, *cell, *room_of, *scal;
    long hslots;
    int32_t *counts;
    const int32_t *positions; uint32_t seed; int32_t *nbr;
};

// coarse cell of point i: round(x / 0.3) per axis, float32 division by float32(0.3), half to even (test_mcpnet.py:86, :98)
__device__ __forceinline__ void mcp_cell_of(const McpArgs &a, int i, int *cx, int *cy, int *cz) {
    const float *p = a.pts + (long)i * a.ld;
    *cx = lrg_voxel_of(p[0], LRG_MCP_RADIUS); *cy = lrg_voxel_of(p[1], LRG_MCP_RADIUS); *cz = lrg_voxel_of(p[2], LRG_MCP_RADIUS);
}

__global__ __launch_bounds__(MCP_THREADS) void mcp_init_kernel(McpArgs a) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < a.hslots) { a.keys[t] = LRG_HASH_EMPTY; a.cnt[t] = 0; a.fill[t] = 0; }
    if (t == a.hslots) a.cnt[t] = 0;
    if (t < 64) a.scal[t] = 0;
    if (t >= a.n) return;
    a.room_of[t] = lrg_room_of(a.room_start, a.n_rooms, (int)t);
    a.cell[t] = -1;
}

__global__ __launch_bounds__(MCP_THREADS) void mcp_insert_kernel(McpArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int r = a.room_of[i];
    int s, e;
    if (!lrg_room_bounds(a.room_start, a.n, r, &s, &e)) return;
    int cx, cy, cz;
    mcp_cell_of(a, i, &cx, &cy, &cz);
    const uint64_t key = lrg_pack_voxel(cx, cy, cz);
    if (key == LRG_HASH_EMPTY) { atomicOr(&a.scal[0], MCP_ST_WINDOW); return; }
    long base; int mask;
    lrg_room_segment(r, s, e, &base, &mask);
    const int h = lrg_room_claim(a.keys + base, mask, key);
    if (h < 0) return;
    a.cell[i] = (int)(base + h);
    atomicAdd(&a.cnt[base + h], 1);
}

__global__ __launch_bounds__(MCP_THREADS) void mcp_fill_kernel(McpArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int h = a.cell[i];
    if (h < 0) return;
    const int pos = atomicAdd(&a.fill[h], 1);
    a.members[a.off[h] + pos] = i;
}

__global__ __launch_bounds__(MCP_THREADS) void mcp_sort_kernel(McpArgs a) {
    const long h = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= a.hslots) return;
    const int c = a.cnt[h];
    if (c < 2) return;
    int32_t *m = a.members + a.off[h];
    for (int x = 1; x < c; ++x) {
        const int v = m[x];
        int y = x - 1;
        while (y >= 0 && m[y] > v) { m[y + 1] = m[y]; --y; }
        m[y + 1] = v;
    }
}

// The 27 cells around point i's own cell in itertools.product order: list start and count of each (count 0 where absent).
// Returns the total, or -1 when the point has no cell (status already set).
__device__ __forceinline__ int mcp_cells(const McpArgs &a, int i, int (&start)[27], int (&count)[27]) {
    const int r = a.room_of[i];
    int s, e;
    if (a.cell[i] < 0 || !lrg_room_bounds(a.room_start, a.n, r, &s, &e)) return -1;
    long base; int mask;
    lrg_room_segment(r, s, e, &base, &mask);
    int cx, cy, cz;
    mcp_cell_of(a, i, &cx, &cy, &cz);
    int total = 0, o = 0;
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz, ++o) {
                const int h = lrg_room_find(a.keys + base, mask, lrg_pack_voxel(cx + dx, cy + dy, cz + dz));
                start[o] = h >= 0 ? a.off[base + h] : 0;
                count[o] = h >= 0 ? a.cnt[base + h] : 0;
                total += count[o];
            }
    return total;
}

__global__ __launch_bounds__(MCP_THREADS) void mcp_count_kernel(McpArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    int start[27], count[27];
    const int c = mcp_cells(a, i, start, count);
    a.counts[i] = c < 0 ? 0 : c;
}

__global__ __launch_bounds__(MCP_THREADS) void mcp_neighbor_kernel(McpArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    int start[27], count[27];
    const int c = mcp_cells(a, i, start, count);
    int32_t *out = a.nbr + (long)i * MCP_K;
    if (c <= 0) {
        for (int j = 0; j < MCP_K; ++j) out[j] = i;
        return;
    }
    const int r = a.room_of[i];
    const uint32_t li = (uint32_t)(i - a.room_start[r]), k0 = a.seed, k1 = (uint32_t)a.rids[r];
    lrg_u32x4 keys = {0u, 0u, 0u, 0u};
    if (!a.positions && c >= MCP_K)
        keys = lrg_philox4x32_10(0u, 0u, li, (LRG_PURPOSE_MCP_NEIGHBOR | LRG_PURPOSE_PERMKEY) & 0xFFu, k0, k1);
    for (int j = 0; j < MCP_K; ++j) {
        int pos;
        if (a.positions) {
            pos = a.positions[(long)i * MCP_K + j];
            if (pos < 0 || pos >= c) { atomicOr(&a.scal[0], MCP_ST_POSITION); out[j] = i; continue; }
        } else if (c >= MCP_K) {
            pos = (int)lrg_feistel_permute((uint32_t)j, (uint32_t)c, keys);          // without replacement: the first 50 of a permutation
        } else {
            const uint32_t w = lrg_rng_word((uint32_t)j, LRG_PURPOSE_MCP_NEIGHBOR, li, 0u, 0u, k0, k1);
            pos = (int)(((uint64_t)w * (uint64_t)c) >> 32);                         // with replacement: 50 independent draws
        }
        int o = 0;
        while (o < 26 && pos >= count[o]) { pos -= count[o]; ++o; }
        out[j] = a.members[start[o] + pos];
    }
}

// ---- the embedding network ----

__global__ __launch_bounds__(64) void mcp_embed_kernel(const float *__restrict__ pts, int ld, int n, const int32_t *__restrict__ nbr,
                                                       const float *__restrict__ W, float *__restrict__ emb, int32_t *status) {
    __shared__ float4 s_k1[MCP_H * 2];                   // K1[0..3][c] | K1[4][c], K1[5][c], b1[c], b2[c]
    __shared__ float s_pool[(MCP_H + 4) * MCP_PTS];      // [k][point]: z, r, g, b, then the pooled 200 (later: the 200 of layer 3)
    __shared__ float s_out[MCP_PTS * 16];
    const int lane = threadIdx.x, h = lane >> 5, rl = lane & 31;
    const int P0 = blockIdx.x * MCP_PTS;
    const int np = n - P0 < MCP_PTS ? n - P0 : MCP_PTS;
    const float4 *k1g = reinterpret_cast<const float4 *>(W + MCP_OFF_K1);
    for (int x = lane; x < MCP_H * 2; x += 64) s_k1[x] = k1g[x];
    for (int x = lane; x < (MCP_H + 4) * MCP_PTS; x += 64) s_pool[x] = 0.f;
    __syncthreads();
    if (lane < 4 * MCP_PTS) {                             // concat([points[i, 2:6], pooled]) (learn_region_grow_util.py:219)
        const int p = lane & 15, q = lane >> 4;
        if (p < np) s_pool[q * MCP_PTS + p] = pts[(long)(P0 + p) * ld + 2 + q];
    }
    unsigned *pool = reinterpret_cast<unsigned *>(s_pool + 4 * MCP_PTS);
    const int rows = np * MCP_K, tiles = (rows + 31) >> 5;
    const float4 *k2 = reinterpret_cast<const float4 *>(W + MCP_OFF_K2) + lane;
    bool bad = false;
    #pragma unroll 1
    for (int tile = 0; tile < tiles; ++tile) {
        asm volatile("" ::: "memory");                    // keep the layer-1 weight reads in the loop (hoisted they would take 800 registers)
        const int row0 = tile * 32, grow = row0 + rl;
        float x[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (grow < rows) {                               // points[nbr, :6] - points[i, :6] (test_mcpnet.py:105-106)
            const int i = P0 + grow / MCP_K;
            int nb = nbr[(long)i * MCP_K + grow % MCP_K];
            if ((unsigned)nb >= (unsigned)n) { bad = true; nb = i; }
            const float *pn = pts + (long)nb * ld, *pi = pts + (long)i * ld;
#pragma unroll
            for (int f = 0; f < 6; ++f) x[f] = __fsub_rn(pn[f], pi[f]);
        }
        // layer 1: relu(x . K1 + b1) for columns 2 s + h -> the A operand of k-step s
        float a[100];
#pragma unroll
        for (int s = 0; s < 100; ++s) {
            const float4 w0 = s_k1[2 * (2 * s + h)], w1 = s_k1[2 * (2 * s + h) + 1];
            float v = __fmul_rn(x[0], w0.x);
            v = __fmaf_rn(x[1], w0.y, v); v = __fmaf_rn(x[2], w0.z, v); v = __fmaf_rn(x[3], w0.w, v);
            v = __fmaf_rn(x[4], w1.x, v); v = __fmaf_rn(x[5], w1.y, v);
            v = __fadd_rn(v, w1.z);
            a[s] = v > 0.f ? v : 0.f;
        }
        // layer 2 on the matrix cores, 32 columns at a time, weights through a ring MCP_FD groups ahead
        float4 bq[MCP_FD];
#pragma unroll
        for (int g = 0; g < MCP_FD; ++g) bq[g] = k2[g * 64];
        const int pl = row0 / MCP_K;                     // the first point of the tile (a tile spans at most two)
        #pragma unroll 1
        for (int t = 0; t < MCP_NT; ++t) {
            const float4 *wp = k2 + (long)t * MCP_KG * 64;
            const float4 *wpn = k2 + (long)(t + 1 < MCP_NT ? t + 1 : t) * MCP_KG * 64;
            f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int g = 0; g < MCP_KG; ++g) {
                const float4 b = bq[g % MCP_FD];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * g + 0], b.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * g + 1], b.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * g + 2], b.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * g + 3], b.w, acc, 0, 0, 0);
                bq[g % MCP_FD] = (g + MCP_FD < MCP_KG) ? wp[(g + MCP_FD) * 64] : wpn[(g + MCP_FD - MCP_KG) * 64];
            }
            // bias, relu, max over the 50 rows of each point (learn_region_grow_util.py:214-218)
            const int col = 32 * t + rl;
            const float bias = col < MCP_H ? s_k1[2 * col + 1].w : 0.f;
            float m0 = 0.f, m1 = 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int rr = row0 + (q & 3) + 8 * (q >> 2) + 4 * h;
                float v = __fadd_rn(acc[q], bias);
                v = v > 0.f ? v : 0.f;
                if (rr < rows) {
                    if (rr / MCP_K == pl) m0 = fmaxf(m0, v); else m1 = fmaxf(m1, v);
                }
            }
            if (col < MCP_H) {
                atomicMax(&pool[col * MCP_PTS + pl], __float_as_uint(m0));
                if (pl + 1 < np && (pl + 1) * MCP_K < row0 + 32) atomicMax(&pool[col * MCP_PTS + pl + 1], __float_as_uint(m1));
            }
        }
    }
    if (bad) atomicOr(status, 1);
    __syncthreads();
    // layer 3: relu(concat . K3 + b3), lane: columns lane + 64 m, all 16 points
    const float *k3 = W + MCP_OFF_K3;
    float acc3[4][MCP_PTS];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int p = 0; p < MCP_PTS; ++p) acc3[m][p] = 0.f;
    #pragma unroll 1
    for (int k = 0; k < MCP_H + 4; ++k) {
        float w[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) w[m] = (lane + 64 * m < MCP_H) ? k3[k * MCP_H + lane + 64 * m] : 0.f;
        const float4 *xin = reinterpret_cast<const float4 *>(s_pool + k * MCP_PTS);
#pragma unroll
        for (int p4 = 0; p4 < 4; ++p4) {
            const float4 v = xin[p4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                acc3[m][4 * p4 + 0] = __fmaf_rn(v.x, w[m], acc3[m][4 * p4 + 0]);
                acc3[m][4 * p4 + 1] = __fmaf_rn(v.y, w[m], acc3[m][4 * p4 + 1]);
                acc3[m][4 * p4 + 2] = __fmaf_rn(v.z, w[m], acc3[m][4 * p4 + 2]);
                acc3[m][4 * p4 + 3] = __fmaf_rn(v.w, w[m], acc3[m][4 * p4 + 3]);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int c = lane + 64 * m;
        if (c < MCP_H) {
            const float b3 = W[MCP_OFF_B3 + c];
#pragma unroll
            for (int p = 0; p < MCP_PTS; ++p) {
                const float v = __fadd_rn(acc3[m][p], b3);
                s_pool[c * MCP_PTS + p] = v > 0.f ? v : 0.f;
            }
        }
    }
    __syncthreads();
    // layer 4: fc3 . K4 + b4, one output (point, e) per lane and pass
    for (int o = lane; o < MCP_PTS * MCP_E; o += 64) {
        const int p = o / MCP_E, e = o % MCP_E;
        float v = 0.f;
        for (int c = 0; c < MCP_H; ++c) v = __fmaf_rn(s_pool[c * MCP_PTS + p], W[MCP_OFF_K4 + c * MCP_E + e], v);
        s_out[p * 16 + e] = __fadd_rn(v, W[MCP_OFF_B4 + e]);
    }
    __syncthreads();
    // tf.nn.l2_normalize(axis=1): x * rsqrt(max(sum(x^2), 1e-12))
    if (lane < np) {
        const float *v = s_out + lane * 16;
        float ss = 0.f;
#pragma unroll
        for (int e = 0; e < MCP_E; ++e) ss = __fmaf_rn(v[e], v[e], ss);
        const float inv = __fdiv_rn(1.f, __fsqrt_rn(fmaxf(ss, 1e-12f)));
#pragma unroll
        for (int e = 0; e < MCP_E; ++e) emb[(long)(P0 + lane) * MCP_E + e] = __fmul_rn(v[e], inv);
    }
}

__global__ __launch_bounds__(MCP_THREADS) void mcp_pack_kernel(const float *k1, const float *b1, const float *k2, const float *b2,
                                                               const float *k3, const float *b3, const float *k4, const float *b4,
                                                               float *out) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= MCP_PACKED) return;
    float v = 0.f;
    if (x < MCP_OFF_K2) {
        const int c = x >> 3, f = x & 7;
        v = f < 6 ? k1[f * MCP_H + c] : (f == 6 ? b1[c] : b2[c]);
    } else if (x < MCP_OFF_K3) {
        const int y = x - MCP_OFF_K2, q = y & 3, l = (y >> 2) & 63, g = (y >> 8) % MCP_KG, t = (y >> 8) / MCP_KG;
        const int k = 8 * g + 2 * q + (l >> 5), col = 32 * t + (l & 31);
        v = col < MCP_H ? k2[k * MCP_H + col] : 0.f;
    } else if (x < MCP_OFF_B3) {
        v = k3[x - MCP_OFF_K3];
    } else if (x < MCP_OFF_K4) {
        v = b3[x - MCP_OFF_B3];
    } else if (x < MCP_OFF_B4) {
        v = k4[x - MCP_OFF_K4];
    } else if (x - MCP_OFF_B4 < MCP_E) {
        v = b4[x - MCP_OFF_B4];
    }
    out[x] = v;
}

static int mcp_args(const float *pts, int ld, const int32_t *room_start, int n_rooms, void *ws, size_t ws_bytes, LrgMcpLayout *L,
                    McpArgs *a) {
    if (n_rooms < 1 || n_rooms > (1 << 20) || !room_start || room_start[0] != 0) return LRG_EINVAL - 81;
    for (int r = 0; r < n_rooms; ++r)
        if (room_start[r + 1] < room_start[r]) return LRG_EINVAL - 81;
    const int n = room_start[n_rooms];
    int rc = mcp_layout(n, n_rooms, L);
    if (rc) return rc;
    if (!ws || (n > 0 && (!pts || ld < 6))) return LRG_EINVAL - 82;
    if (ws_bytes < L->total || ((uintptr_t)ws & 255)) return LRG_EINVAL - 83;
    char *w = static_cast<char *>(ws);
    a->pts = pts; a->ld = ld; a->n_rooms = n_rooms; a->n = n;
    a->room_start = reinterpret_cast<int32_t *>(w + L->rooms); a->rids = reinterpret_cast<int32_t *>(w + L->rids);
    a->keys = reinterpret_cast<uint64_t *>(w + L->keys); a->cnt = reinterpret_cast<int32_t *>(w + L->cnt);
    a->off = reinterpret_cast<int32_t *>(w + L->off); a->fill = reinterpret_cast<int32_t *>(w + L->fill);
    a->members = reinterpret_cast<int32_t *>(w + L->members); a->cell = reinterpret_cast<int32_t *>(w + L->cell);
    a->room_of = reinterpret_cast<int32_t *>(w + L->room_of); a->scal = reinterpret_cast<int32_t *>(w + L->scal);
    a->hslots = L->hslots; a->counts = nullptr; a->positions = nullptr; a->seed = 0; a->nbr = nullptr;
    return 0;
}

extern "C" {

size_t lrg_mcp_workspace_bytes(int n_points, int n_rooms) {
    LrgMcpLayout L;
    if (mcp_layout(n_points, n_rooms, &L)) return 0;
    return L.total;
}

int lrg_mcp_candidates(const float *pts, int ld, const int32_t *room_start, int n_rooms, void *ws, size_t ws_bytes, int32_t *counts,
                       void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LrgMcpLayout L;
    McpArgs a;
    int rc = mcp_args(pts, ld, room_start, n_rooms, ws, ws_bytes, &L, &a);
    if (rc) return rc;
    if (!counts && a.n > 0) return LRG_EINVAL - 82;
    a.counts = counts;
    LRG_HIP_CHECK(hipMemcpyAsync(const_cast<int32_t *>(a.room_start), room_start, (size_t)(n_rooms + 1) * sizeof(int32_t),
                                 hipMemcpyHostToDevice, st));
    const long init_n = L.hslots + 1 > (long)a.n + 64 ? L.hslots + 1 : (long)a.n + 64;
    const int gi = (int)((init_n + MCP_THREADS - 1) / MCP_THREADS);
    const int gn = (int)(((long)a.n + MCP_THREADS - 1) / MCP_THREADS);
    const int gh = (int)((L.hslots + MCP_THREADS - 1) / MCP_THREADS);
    hipLaunchKernelGGL(mcp_init_kernel, dim3(gi), dim3(MCP_THREADS), 0, st, a);
    if (a.n > 0) hipLaunchKernelGGL(mcp_insert_kernel, dim3(gn), dim3(MCP_THREADS), 0, st, a);
    // cnt[0 .. hslots] into off: the start of each cell's member list
    if ((rc = lrg_exscan_i32(a.cnt, L.hslots + 1, reinterpret_cast<int32_t *>(static_cast<char *>(ws) + L.bsum), a.off, st))) return rc;
    if (a.n > 0) {
        hipLaunchKernelGGL(mcp_fill_kernel, dim3(gn), dim3(MCP_THREADS), 0, st, a);
        hipLaunchKernelGGL(mcp_sort_kernel, dim3(gh), dim3(MCP_THREADS), 0, st, a);
        hipLaunchKernelGGL(mcp_count_kernel, dim3(gn), dim3(MCP_THREADS), 0, st, a);
    }
    LRG_LAUNCH_CHECK();
    return 0;
}

int lrg_mcp_neighbors(const float *pts, int ld, const int32_t *room_start, int n_rooms, void *ws, size_t ws_bytes,
                      const int32_t *positions, uint32_t seed, const int32_t *room_ids, int32_t *nbr, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    LrgMcpLayout L;
    McpArgs a;
    int rc = mcp_args(pts, ld, room_start, n_rooms, ws, ws_bytes, &L, &a);
    if (rc) return rc;
    if (!nbr && a.n > 0) return LRG_EINVAL - 82;
    if (!positions && !room_ids) return LRG_EINVAL - 84;
    a.positions = positions; a.seed = seed; a.nbr = nbr;
    if (!positions)
        LRG_HIP_CHECK(hipMemcpyAsync(const_cast<int32_t *>(a.rids), room_ids, (size_t)n_rooms * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (a.n > 0) hipLaunchKernelGGL(mcp_neighbor_kernel, dim3((a.n + MCP_THREADS - 1) / MCP_THREADS), dim3(MCP_THREADS), 0, st, a);
    LRG_LAUNCH_CHECK();
    return 0;
}

int lrg_mcp_status(const void *ws, int n_points, int n_rooms, int32_t *host_status, void *stream) {
    LrgMcpLayout L;
    int rc = mcp_layout(n_points, n_rooms, &L);
    if (rc) return rc;
    if (!ws || !host_status) return LRG_EINVAL - 82;
    LRG_HIP_CHECK(hipMemcpyAsync(host_status, static_cast<const char *>(ws) + L.scal, sizeof(int32_t), hipMemcpyDeviceToHost,
                                 (hipStream_t)stream));
    LRG_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

size_t lrg_mcp_packed_floats(void) { return MCP_PACKED; }

int lrg_mcp_pack_weights(const float *k1, const float *b1, const float *k2, const float *b2, const float *k3, const float *b3,
                         const float *k4, const float *b4, float *packed, void *stream) {
    if (!k1 || !b1 || !k2 || !b2 || !k3 || !b3 || !k4 || !b4 || !packed) return LRG_EINVAL - 85;
    hipLaunchKernelGGL(mcp_pack_kernel, dim3((MCP_PACKED + MCP_THREADS - 1) / MCP_THREADS), dim3(MCP_THREADS), 0, (hipStream_t)stream,
                       k1, b1, k2, b2, k3, b3, k4, b4, packed);
    LRG_LAUNCH_CHECK();
    return 0;
}

int lrg_mcp_embed(const float *pts, int ld, int n_points, const int32_t *nbr, const float *packed, float *emb, int32_t *status,
                  void *stream) {
    if (n_points < 0 || n_points > (1 << 26)) return LRG_EINVAL - 86;
    if (n_points == 0) return 0;
    if (!pts || ld < 6 || !nbr || !packed || !emb || !status) return LRG_EINVAL - 87;
    hipLaunchKernelGGL(mcp_embed_kernel, dim3((n_points + MCP_PTS - 1) / MCP_PTS), dim3(64), 0, (hipStream_t)stream,
                       pts, ld, n_points, nbr, packed, emb, status);
    LRG_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
