// Training MCPNet (train_mcpnet.py:187-205) on gfx950: the forward pass that keeps its layers, and triplet_semihard_loss
// (metric_loss_ops.py:157-236 over pairwise_distance(squared=True), :40-81) with its gradient down to fc4.  The backward pass of the
// network itself runs on lrg_train.hip's kernels, sequenced by learn_region_grow_amd/mcpnet_train.py.  DESIGN.md §3.17.
//
// Forward (lrg_mcp_embed_train).  mcp_embed_kernel of lrg_mcpnet.hip with the rows given (the staged float32 differences) and every
// layer stored.  A row's bits depend on its own k order alone -- the layer-1 FMA chain, the 100 k-steps of v_mfma_f32_32x32x2_f32 per
// column tile in ascending k, the FMA chains of layers 3 and 4, the normalisation -- and those are restated here unchanged, so emb
// equals lrg_mcp_embed's bit for bit whatever the grouping.  One wavefront takes LRG_MCP_TRAIN_POINTS = 2 points = 100 rows = 4
// row tiles of 32 (28 padding rows), so a batch of 256 is 128 workgroups instead of inference's 16.
//
// Loss (lrg_mcp_triplet_semihard), four launches, nothing added atomically:
//   dist    D_an = max((sq_a + sq_n) - 2 dot_an, 0), diagonal 0; a row's count of positives
//   mine    one workgroup per anchor a, thread n = column n.  For every positive p in ascending order the workgroup reduces
//           y_n = (D_an - M_a) mask_n (mask_n: label differs and D_an > D_ap; M_a the row maximum) to its minimum, the number of
//           entries equal to it and how many of those lie in the mask -- masked_minimum (:138-154); S_ap = min + M_a, or
//           negatives_inside (masked_maximum :119-135 of the row over label-differs) when the mask is empty (:216).  Where
//           margin + (D_ap - S_ap) >= 0 (tf.maximum sends the gradient to x where x >= y) thread n adds its share to its own G_an:
//             + g at n = p;  - g / ties at the tied entries inside the mask (reduce_min: equal shares among equal entries; the
//             entries outside the mask are 0 and tie with a minimum of 0, their shares die in the mask's product);
//             (- g + inside g / ties) / |{D_an = M_a}| at the row's maxima (the two uses of axis_maximums; 0 unless the minimum is 0)
//           with g = 1 / num_positives, and after the loop the same for negatives_inside with the sum of its pairs' - g.
//           dD_an = G_an where D_an > 0 and n != a (:61 maximum, :73 error mask, :80 off-diagonal), else 0.
//   grad    dE_i = 2 sum_j (dD_ij + dD_ji)(e_i - e_j), ascending j; then dfc4 = (dE - e (dE . e)) / sqrt(max(|fc4|^2, 1e-12)),
//           without the second term where |fc4|^2 < 1e-12 (tf.nn.l2_normalize: x * rsqrt(maximum(sum x^2, 1e-12)))
//   stats   the rows' four sums in ascending row order, in double
#include "lrg_mcp_layout.h"

#define MCPT_PTS LRG_MCP_TRAIN_POINTS
#define MCPL_MAXB LRG_MCP_TRIPLET_MAX_B
#define MCPL_WAVES (MCPL_MAXB / 64)

__global__ __launch_bounds__(64) void mcp_embed_train_kernel(const float *__restrict__ x, const float *__restrict__ ctr, int n,
                                                             const float *__restrict__ W, float *__restrict__ h1, float *__restrict__ h2,
                                                             float *__restrict__ cat, float *__restrict__ fc3, float *__restrict__ fc4,
                                                             float *__restrict__ emb) {
    __shared__ float4 s_k1[MCP_H * 2];                   // K1[0..3][c] | K1[4][c], K1[5][c], b1[c], b2[c]
    __shared__ float s_pool[(MCP_H + 4) * MCPT_PTS];     // [k][point]: z, r, g, b, then the pooled 200 (later: the 200 of layer 3)
    __shared__ float s_out[MCPT_PTS * 16];
    const int lane = threadIdx.x, h = lane >> 5, rl = lane & 31;
    const int P0 = blockIdx.x * MCPT_PTS;
    const int np = n - P0 < MCPT_PTS ? n - P0 : MCPT_PTS;
    const float4 *k1g = reinterpret_cast<const float4 *>(W + MCP_OFF_K1);
    for (int i = lane; i < MCP_H * 2; i += 64) s_k1[i] = k1g[i];
    for (int i = lane; i < (MCP_H + 4) * MCPT_PTS; i += 64) s_pool[i] = 0.f;
    __syncthreads();
    if (lane < 4 * MCPT_PTS) {                            // concat([input_pl, pooled]) (learn_region_grow_util.py:217)
        const int p = lane % MCPT_PTS, q = lane / MCPT_PTS;
        if (p < np) s_pool[q * MCPT_PTS + p] = ctr[(long)(P0 + p) * 4 + q];
    }
    unsigned *pool = reinterpret_cast<unsigned *>(s_pool + 4 * MCPT_PTS);
    const int rows = np * MCP_K, tiles = (rows + 31) >> 5;
    const float4 *k2 = reinterpret_cast<const float4 *>(W + MCP_OFF_K2) + lane;
    #pragma unroll 1
    for (int tile = 0; tile < tiles; ++tile) {
        asm volatile("" ::: "memory");                    // keep the layer-1 weight reads in the loop
        const int row0 = tile * 32, grow = row0 + rl;
        float xr[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (grow < rows) {
            const float *px = x + ((long)P0 * MCP_K + grow) * 6;
#pragma unroll
            for (int f = 0; f < 6; ++f) xr[f] = px[f];
        }
        // layer 1: relu(x . K1 + b1) for columns 2 s + h -> the A operand of k-step s
        float a[100];
#pragma unroll
        for (int s = 0; s < 100; ++s) {
            const float4 w0 = s_k1[2 * (2 * s + h)], w1 = s_k1[2 * (2 * s + h) + 1];
            float v = __fmul_rn(xr[0], w0.x);
            v = __fmaf_rn(xr[1], w0.y, v); v = __fmaf_rn(xr[2], w0.z, v); v = __fmaf_rn(xr[3], w0.w, v);
            v = __fmaf_rn(xr[4], w1.x, v); v = __fmaf_rn(xr[5], w1.y, v);
            v = __fadd_rn(v, w1.z);
            a[s] = v > 0.f ? v : 0.f;
        }
        if (h1 && grow < rows) {
            float *o = h1 + ((long)P0 * MCP_K + grow) * MCP_H + h;
#pragma unroll
            for (int s = 0; s < 100; ++s) o[2 * s] = a[s];
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
            // bias, relu, max over the 50 rows of each point (learn_region_grow_util.py:214-216)
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
                    if (h2 && col < MCP_H) h2[((long)P0 * MCP_K + rr) * MCP_H + col] = v;
                }
            }
            if (col < MCP_H) {
                atomicMax(&pool[col * MCPT_PTS + pl], __float_as_uint(m0));
                if (pl + 1 < np && (pl + 1) * MCP_K < row0 + 32) atomicMax(&pool[col * MCPT_PTS + pl + 1], __float_as_uint(m1));
            }
        }
    }
    __syncthreads();
    if (cat)
        for (int i = lane; i < (MCP_H + 4) * MCPT_PTS; i += 64) {
            const int k = i / MCPT_PTS, p = i % MCPT_PTS;
            if (p < np) cat[(long)(P0 + p) * (MCP_H + 4) + k] = s_pool[i];
        }
    // layer 3: relu(concat . K3 + b3), lane: columns lane + 64 m, both points
    const float *k3 = W + MCP_OFF_K3;
    float acc3[4][MCPT_PTS];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int p = 0; p < MCPT_PTS; ++p) acc3[m][p] = 0.f;
    #pragma unroll 4
    for (int k = 0; k < MCP_H + 4; ++k) {
        float w[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) w[m] = (lane + 64 * m < MCP_H) ? k3[k * MCP_H + lane + 64 * m] : 0.f;
#pragma unroll
        for (int p = 0; p < MCPT_PTS; ++p) {
            const float v = s_pool[k * MCPT_PTS + p];
#pragma unroll
            for (int m = 0; m < 4; ++m) acc3[m][p] = __fmaf_rn(v, w[m], acc3[m][p]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int c = lane + 64 * m;
        if (c < MCP_H) {
            const float b3 = W[MCP_OFF_B3 + c];
#pragma unroll
            for (int p = 0; p < MCPT_PTS; ++p) {
                float v = __fadd_rn(acc3[m][p], b3);
                v = v > 0.f ? v : 0.f;
                s_pool[c * MCPT_PTS + p] = v;
                if (fc3 && p < np) fc3[(long)(P0 + p) * MCP_H + c] = v;
            }
        }
    }
    __syncthreads();
    // layer 4: fc3 . K4 + b4, one output (point, e) per lane
    for (int o = lane; o < MCPT_PTS * MCP_E; o += 64) {
        const int p = o / MCP_E, e = o % MCP_E;
        float v = 0.f;
        for (int c = 0; c < MCP_H; ++c) v = __fmaf_rn(s_pool[c * MCPT_PTS + p], W[MCP_OFF_K4 + c * MCP_E + e], v);
        v = __fadd_rn(v, W[MCP_OFF_B4 + e]);
        s_out[p * 16 + e] = v;
        if (fc4 && p < np) fc4[(long)(P0 + p) * MCP_E + e] = v;
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

// ---- the loss ----
__device__ __forceinline__ float mcpl_sq(const float *e) {
    float s = __fmul_rn(e[0], e[0]);
#pragma unroll
    for (int k = 1; k < MCP_E; ++k) s = __fadd_rn(s, __fmul_rn(e[k], e[k]));
    return s;
}

// rowstat[a][1] = the positives of row a; D[a][n]
__global__ __launch_bounds__(MCPL_MAXB) void mcpl_dist_kernel(const float *__restrict__ emb, const int32_t *__restrict__ labels, int B,
                                                              float *__restrict__ D, double *__restrict__ rowstat) {
    __shared__ int s_cnt[MCPL_WAVES];
    const int a = blockIdx.x, n = threadIdx.x;
    int pos = 0;
    if (n < B) {
        float ea[MCP_E], en[MCP_E];
#pragma unroll
        for (int k = 0; k < MCP_E; ++k) { ea[k] = emb[a * MCP_E + k]; en[k] = emb[n * MCP_E + k]; }
        float dot = __fmul_rn(ea[0], en[0]);
#pragma unroll
        for (int k = 1; k < MCP_E; ++k) dot = __fadd_rn(dot, __fmul_rn(ea[k], en[k]));
        const float d = fmaxf(__fsub_rn(__fadd_rn(mcpl_sq(ea), mcpl_sq(en)), __fmul_rn(2.f, dot)), 0.f);
        D[(long)a * B + n] = n == a ? 0.f : d;
        pos = n != a && labels[n] == labels[a];
    }
    for (int o = 32; o > 0; o >>= 1) pos += __shfl_xor(pos, o);
    if ((n & 63) == 0) s_cnt[n >> 6] = pos;
    __syncthreads();
    if (n == 0) {
        int t = 0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += s_cnt[w];
        rowstat[a * 4 + 1] = (double)t;
    }
}

// An extremum of the workgroup's values with the number of entries equal to it (cnt) and how many of those carry a flag (k).
struct McplRed { float v; int cnt, k; };

template <bool IS_MIN>
__device__ __forceinline__ McplRed mcpl_merge(McplRed x, McplRed y) {
    const bool better = IS_MIN ? y.v < x.v : y.v > x.v;
    if (better) return y;
    if (y.v == x.v) { x.cnt += y.cnt; x.k += y.k; }
    return x;
}

// Every thread passes (value, live, flag); entries that are not live (n >= B) do not count.  buf: one of two LDS areas used in turn,
// so one barrier per reduction is enough.  The merge is exact (comparisons and integer sums), so its order does not matter.
template <bool IS_MIN>
__device__ __forceinline__ McplRed mcpl_reduce(float v, bool live, bool flag, McplRed *buf) {
    McplRed r;
    r.v = live ? v : (IS_MIN ? INFINITY : -INFINITY);
    r.cnt = live ? 1 : 0;
    r.k = live && flag ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) {
        McplRed y;
        y.v = __shfl_xor(r.v, o); y.cnt = __shfl_xor(r.cnt, o); y.k = __shfl_xor(r.k, o);
        r = mcpl_merge<IS_MIN>(r, y);
    }
    if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = r;
    __syncthreads();
    McplRed t = buf[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) t = mcpl_merge<IS_MIN>(t, buf[w]);
    return t;
}

__global__ __launch_bounds__(MCPL_MAXB) void mcpl_mine_kernel(const float *__restrict__ D, const int32_t *__restrict__ labels, int B,
                                                              float margin, float *__restrict__ dD, double *__restrict__ rowstat) {
    __shared__ float s_d[MCPL_MAXB];
    __shared__ int32_t s_lab[MCPL_MAXB];
    __shared__ McplRed s_red[2][MCPL_WAVES];
    __shared__ double s_np[MCPL_WAVES];
    const int a = blockIdx.x, n = threadIdx.x;
    const bool live = n < B;
    const float d = live ? D[(long)a * B + n] : 0.f;
    const int32_t lab = live ? labels[n] : 0;
    double posr = live ? rowstat[n * 4 + 1] : 0.0;                 // integers below 2^20: any order adds them exactly
    for (int o = 32; o > 0; o >>= 1) posr += __shfl_xor(posr, o);
    if ((n & 63) == 0) s_np[n >> 6] = posr;
    if (live) { s_d[n] = d; s_lab[n] = lab; }
    __syncthreads();
    double npos = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) npos += s_np[w];
    const int32_t la = s_lab[a];
    const bool neg = live && lab != la;
    const float g = npos > 0.0 ? __fdiv_rn(1.f, (float)npos) : 0.f;
    int turn = 0;
    const McplRed rmax = mcpl_reduce<false>(d, live, false, s_red[turn]); turn ^= 1;       // M_a and its ties
    const McplRed rmin = mcpl_reduce<true>(d, live, false, s_red[turn]); turn ^= 1;        // the row minimum and its ties
    const float Ma = rmax.v, ma = rmin.v;
    // negatives_inside: masked_maximum(D, adjacency_not) (:214-215)
    const float z = neg ? __fsub_rn(d, ma) : 0.f;
    const McplRed rin = mcpl_reduce<false>(z, live, neg, s_red[turn]); turn ^= 1;
    const float inside = __fadd_rn(rin.v, ma);
    float G = 0.f, g_inside = 0.f;
    double loss = 0.0;
    int active = 0, fallback = 0;
    for (int p = 0; p < B; ++p) {
        if (p == a || s_lab[p] != la) continue;
        const float dap = s_d[p];
        const bool in = neg && d > dap;                            // the mask of :193-197 for the pair (a, p)
        const float y = in ? __fsub_rn(d, Ma) : 0.f;
        const McplRed r = mcpl_reduce<true>(y, live, in, s_red[turn]); turn ^= 1;
        const bool outside = r.k > 0;
        const float S = outside ? __fadd_rn(r.v, Ma) : inside;
        const float v = __fadd_rn(margin, __fsub_rn(dap, S));
        fallback += !outside;
        if (!(v >= 0.f)) continue;
        ++active;
        loss += (double)fmaxf(v, 0.f);
        if (n == p) G = __fadd_rn(G, g);
        if (outside) {
            const float share = __fdiv_rn(g, (float)r.cnt);
            if (in && y == r.v) G = __fsub_rn(G, share);
            const float gm = __fdiv_rn(__fadd_rn(-g, __fmul_rn((float)r.k, share)), (float)rmax.cnt);
            if (live && d == Ma) G = __fadd_rn(G, gm);
        } else {
            g_inside = __fsub_rn(g_inside, g);
        }
    }
    {   // the gradient of negatives_inside: its maximum's ties, then the row minimum's
        const float share = __fdiv_rn(g_inside, (float)rin.cnt);
        if (neg && z == rin.v) G = __fadd_rn(G, share);
        const float gm = __fdiv_rn(__fsub_rn(g_inside, __fmul_rn((float)rin.k, share)), (float)rmin.cnt);
        if (live && d == ma) G = __fadd_rn(G, gm);
    }
    if (live) dD[(long)a * B + n] = (d > 0.f && n != a) ? G : 0.f;
    if (n == 0) {
        rowstat[a * 4 + 0] = loss;
        rowstat[a * 4 + 2] = (double)active;
        rowstat[a * 4 + 3] = (double)fallback;
    }
}

__global__ __launch_bounds__(64) void mcpl_grad_kernel(const float *__restrict__ fc4, const float *__restrict__ emb,
                                                       const float *__restrict__ dD, int B, float *__restrict__ dfc4) {
    __shared__ float s_de[16];
    const int i = blockIdx.x, e = threadIdx.x;
    if (e < MCP_E) {
        const float ei = emb[i * MCP_E + e];
        float acc = 0.f;
        for (int j = 0; j < B; ++j) {
            const float w = __fadd_rn(dD[(long)i * B + j], dD[(long)j * B + i]);
            acc = __fmaf_rn(w, __fsub_rn(ei, emb[j * MCP_E + e]), acc);
        }
        s_de[e] = __fmul_rn(2.f, acc);
    }
    __syncthreads();
    if (e < MCP_E) {
        float ss = 0.f, dot = 0.f;
        for (int k = 0; k < MCP_E; ++k) {
            const float x = fc4[i * MCP_E + k];
            ss = __fmaf_rn(x, x, ss);
            dot = __fmaf_rn(s_de[k], emb[i * MCP_E + k], dot);
        }
        const float inv = __fdiv_rn(1.f, __fsqrt_rn(fmaxf(ss, 1e-12f)));
        const float t = ss >= 1e-12f ? __fmul_rn(emb[i * MCP_E + e], dot) : 0.f;
        dfc4[i * MCP_E + e] = __fmul_rn(__fsub_rn(s_de[e], t), inv);
    }
}

__global__ __launch_bounds__(64) void mcpl_stats_kernel(const double *__restrict__ rowstat, int B, double *__restrict__ stats) {
    const int q = threadIdx.x;
    if (q >= 4) return;
    double s = 0.0;
    for (int a = 0; a < B; ++a) s += rowstat[a * 4 + q];
    stats[q] = s;
}

extern "C" {

int lrg_mcp_embed_train(const float *x, const float *c, int n, const float *packed, float *h1, float *h2, float *cat, float *fc3,
                        float *fc4, float *emb, void *stream) {
    if (n < 0 || n > (1 << 22)) return LRG_EINVAL - 90;
    if (n == 0) return 0;
    if (!x || !c || !packed || !emb) return LRG_EINVAL - 90;
    hipLaunchKernelGGL(mcp_embed_train_kernel, dim3((n + MCPT_PTS - 1) / MCPT_PTS), dim3(64), 0, (hipStream_t)stream, x, c, n, packed,
                       h1, h2, cat, fc3, fc4, emb);
    LRG_LAUNCH_CHECK();
    return 0;
}

size_t lrg_mcp_triplet_workspace_doubles(int B) { return B < 2 || B > MCPL_MAXB ? 0 : (size_t)4 * B; }

int lrg_mcp_triplet_semihard(const float *fc4, const float *emb, const int32_t *labels, int B, float margin, float *D, float *dD,
                             float *dfc4, double *stats, double *ws, void *stream) {
    if (B < 2 || B > MCPL_MAXB) return LRG_EINVAL - 91;
    if (!fc4 || !emb || !labels || !D || !dD || !dfc4 || !stats || !ws) return LRG_EINVAL - 92;
    hipStream_t st = (hipStream_t)stream;
    const int threads = (B + 63) / 64 * 64;
    hipLaunchKernelGGL(mcpl_dist_kernel, dim3(B), dim3(threads), 0, st, emb, labels, B, D, ws);
    hipLaunchKernelGGL(mcpl_mine_kernel, dim3(B), dim3(threads), 0, st, D, labels, B, margin, dD, ws);
    hipLaunchKernelGGL(mcpl_grad_kernel, dim3(B), dim3(64), 0, st, fc4, emb, dD, B, dfc4);
    hipLaunchKernelGGL(mcpl_stats_kernel, dim3(1), dim3(64), 0, st, ws, B, stats);
    LRG_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
