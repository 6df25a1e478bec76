// The plain PointNet of the reference's benchmarks.py --mode pointnet (train_pointnet.py:31-99) for gfx950, in two kernels.
//
// Both are built like pn2_mlp_kernel (lrg_pointnet2.hip): a workgroup owns one tile of 32 rows in LDS, act[32][ldw], and carries it
// through its layers on v_mfma_f32_32x32x2_f32 without leaving the CU.  The output's 32-column tiles are dealt to the W wavefronts
// round robin (tile t to wavefront t mod W).  A hidden layer is one pass, because its output replaces its input in LDS, so the
// accumulators hold the whole layer; the last layer of a stack leaves the CU, so it takes as many passes as it has columns for.
// Features: W = 4, four tiles per wavefront and pass = 64 accumulator registers per lane, the 1024 columns of the last layer in two
// passes of 512.  (A hidden conv layer wider than 512, which neither network of the reference has, selects an instantiation with eight
// tiles = 128 accumulator registers per lane.)  Head: W = 8, two tiles per wavefront and pass -- its rows fill the CU's LDS, and the
// one resident workgroup then still brings two wavefronts per SIMD (0.32 -> 0.48 of the fp32 matrix peak).
// A operand: one ds_read_b128 per lane per four k-steps (row stride ldw = width + 4 floats: the 16 lanes of a b128 lane group hit 16
// distinct 4-bank sets).  B operand: the weights in operand order (lrg_mlp_pack.h), one global_load_dwordx4 per lane per four k-steps,
// fetched four groups ahead.  The sum over k runs in one fixed order per output value; bias, batch norm and ReLU are separate float32
// roundings (-ffp-contract=off).
//
//   pn_features_kernel  :49-54 and the pool of :56.  x [cells,1024,6] -> conv[0] .. conv[last], ReLU after each.  conv[1] goes to `skip`
//                       on the way through, the last layer's rows to `last` (if given) and the maximum over the tile's 32 rows by an
//                       integer atomicMax on the bits of the non-negative values to `pooled` (zeroed by the entry point): a maximum
//                       does not depend on the order, so the 32 tiles of a cell give the same bits however they are scheduled.
//   pn_head_kernel      :57-99 at inference.  Rows concat(last[p] - pooled[cell], skip[p]) (float32 subtraction; :57-59 tiles the
//                       pooled row to every row, tests/test_pointnet_host.py; never written to memory), the hidden fc layers
//                       relu((x W + b) * scale[p][c] + shift[p][c]) with p the row's position in its cell (the batch norm of :63-84
//                       has moments over the batch axis only, so its moving averages are [1024, c] tables; folded at load), the final
//                       layer x W + b to out [cells,1024,num_class].
// LDS, dynamic: 32 * (widest layer input + 4) * 4 bytes.  Features: 131.6 KB at most (a 1024-wide hidden layer), 16.9 KB for the widths
// [64,64,64,128,1024] and [64,64,128,512] (the last layer never returns to LDS).  Head: 139.8 KB for the 1088-wide concat, 74.2 KB for
// 576; the concat is limited to PN_MAX_CONCAT = 1248 floats (160 256 of the CU's 163 840 bytes).
#include "lrg_common.h"
#include "lrg_mlp_pack.h"

#define PN_THREADS 256
#define PN_ROWS 32
#define PN_CELL_ROWS 1024
#define PN_CELL_TILES (PN_CELL_ROWS / PN_ROWS)
#define PN_IN 6
#define PN_MAX_CONV 5
#define PN_MIN_CONV 2
#define PN_MAX_FC 3
#define PN_MIN_FC 2
#define PN_MAX_K 2048                        // a packed layer's inputs ...
#define PN_MAX_N 1024                        // ... and outputs
#define PN_MAX_CONV_WIDTH 1024
#define PN_MAX_FC_WIDTH 512
#define PN_MAX_CONCAT 1248                   // 32 * (1248 + 4) * 4 = 160 256 bytes of the CU's 163 840
#define PN_MAX_CELLS (1 << 20)

typedef float pn_f32x16 __attribute__((ext_vector_type(16)));

struct PnLayers {
    int n_layers, ldw;
    int kpad[PN_MAX_CONV], nout[PN_MAX_CONV], npad[PN_MAX_CONV];
    long woff[PN_MAX_CONV];
    const float *packed;
};

struct PnFeatArgs {
    PnLayers l;
    const float *x; float *skip, *last; int *pooled;
};

struct PnHeadArgs {
    PnLayers l;
    const float *last, *skip, *pooled, *bn; float *out;
    int c_last, c_skip;
    long bnoff[PN_MAX_FC];
};

// One pass of a layer's products for this wavefront's column tiles: acc[u] = act[32][kpad] x W[:, 32 t ..][32], t = t0 + w + W u
// (W wavefronts in the workgroup).
template <int U, int W>
__device__ __forceinline__ void pn_gemm(const float *ap, const float4 *wl, int G, int nt, int t0, int w, int lane, pn_f32x16 (&acc)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int t = t0 + w + W * u;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[u][q] = 0.f;
        if (t < nt) {                                                    // the same for every lane of the wavefront
            const float4 *wp = wl + (long)t * G * 64 + lane;
            float4 bq[4], bn[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) bq[i] = wp[i * 64];
            #pragma unroll 1
            for (int g0 = 0; g0 < G; g0 += 4) {
                const int gn = g0 + 4 < G ? g0 + 4 : g0;                 // the last round reloads its own groups (unused)
#pragma unroll
                for (int i = 0; i < 4; ++i) bn[i] = wp[(gn + i) * 64];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float4 av = *reinterpret_cast<const float4 *>(ap + 8 * (g0 + i));
                    acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bq[i].x, acc[u], 0, 0, 0);
                    acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bq[i].y, acc[u], 0, 0, 0);
                    acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bq[i].z, acc[u], 0, 0, 0);
                    acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bq[i].w, acc[u], 0, 0, 0);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) bq[i] = bn[i];
            }
        }
    }
}

// accumulator register q of a lane of half h holds tile row (q & 3) + 8 (q >> 2) + 4 h
__device__ __forceinline__ int pn_acc_row(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }

// U: column tiles per wavefront and pass.  A hidden layer is one pass (its output replaces its input in LDS, so the accumulators hold
// the whole layer): 4 U tiles, 128 U columns at most.  The last layer's rows leave the CU, so it takes as many passes as it needs.
template <int U>
__global__ __launch_bounds__(PN_THREADS, U == 4 ? 2 : 1) void pn_features_kernel(PnFeatArgs a) {
    extern __shared__ __attribute__((aligned(16))) float pn_act[];       // [32][ldw]
    float *act = pn_act;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, rl = lane & 31;
    const long tile = blockIdx.x, row0 = tile * PN_ROWS, cell = tile / PN_CELL_TILES;
    const int ldw = a.l.ldw;
    for (int e = tid; e < PN_ROWS * 32; e += PN_THREADS) {               // kpad[0] == 32
        const int row = e >> 5, col = e & 31;
        act[row * ldw + col] = col < PN_IN ? a.x[(row0 + row) * PN_IN + col] : 0.f;
    }
    __syncthreads();
    const float *ap = act + rl * ldw + 4 * h;
    #pragma unroll 1
    for (int L = 0; L < a.l.n_layers; ++L) {
        const int G = a.l.kpad[L] >> 3, nt = a.l.npad[L] >> 5, n = a.l.nout[L];     // n is a multiple of 32: every column is real
        const float4 *wl = reinterpret_cast<const float4 *>(a.l.packed + a.l.woff[L]);
        const float *bias = a.l.packed + a.l.woff[L] + (long)a.l.kpad[L] * a.l.npad[L];
        pn_f32x16 acc[U];
        if (L < a.l.n_layers - 1) {
            pn_gemm<U, 4>(ap, wl, G, nt, 0, w, lane, acc);
            __syncthreads();                                             // every wavefront has read the layer's input
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = w + 4 * u;
                if (t < nt) {
                    const int col = 32 * t + rl;
                    const float bv = bias[col];
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int rr = pn_acc_row(q, h);
                        float v = __fadd_rn(acc[u][q], bv);
                        v = v > 0.f ? v : 0.f;
                        act[rr * ldw + col] = v;
                        if (L == 1) a.skip[(row0 + rr) * n + col] = v;
                    }
                }
            }
            __syncthreads();
        } else {
            #pragma unroll 1
            for (int t0 = 0; t0 < nt; t0 += 4 * U) {
                pn_gemm<U, 4>(ap, wl, G, nt, t0, w, lane, acc);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int t = t0 + w + 4 * u;
                    if (t < nt) {
                        const int col = 32 * t + rl;
                        const float bv = bias[col];
                        float mx = 0.f;                                  // ReLU output: the maximum is >= 0
#pragma unroll
                        for (int q = 0; q < 16; ++q) {
                            const long i = row0 + pn_acc_row(q, h);
                            float v = __fadd_rn(acc[u][q], bv);
                            v = v > 0.f ? v : 0.f;
                            if (L == 1) a.skip[i * n + col] = v;         // a stack of two layers: conv[1] is the last
                            if (a.last) a.last[i * n + col] = v;
                            mx = fmaxf(mx, v);
                        }
                        mx = fmaxf(mx, __shfl_xor(mx, 32));
                        if (h == 0) atomicMax(a.pooled + cell * n + col, __float_as_int(mx));    // mx >= +0: the integer order is the float order
                    }
                }
            }
        }
    }
}

// The head's workgroup is eight wavefronts: its 1088-wide rows fill the CU's LDS, so the one resident workgroup brings the two
// wavefronts per SIMD that hide each other's operand loads.  Tile t to wavefront t mod 8, two per wavefront and pass.
#define PN_HEAD_THREADS 512
#define PN_HEAD_WAVES (PN_HEAD_THREADS / 64)
#define PN_HEAD_U 2                          // hidden fc layers: 512 columns at most = 16 tiles

__global__ __launch_bounds__(PN_HEAD_THREADS, 2) void pn_head_kernel(PnHeadArgs a) {
    extern __shared__ __attribute__((aligned(16))) float pn_act[];       // [32][ldw]
    float *act = pn_act;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, rl = lane & 31;
    const long tile = blockIdx.x, row0 = tile * PN_ROWS, cell = tile / PN_CELL_TILES;
    const int p0 = (int)(tile % PN_CELL_TILES) * PN_ROWS;                // the tile's first row position in its cell
    const int ldw = a.l.ldw, cl = a.c_last, cs = a.c_skip, k0 = cl + cs; // k0 is a multiple of 32
    const float *pool = a.pooled + cell * cl;
    for (int e = tid; e < PN_ROWS * k0; e += PN_HEAD_THREADS) {
        const int row = e / k0, col = e - row * k0;
        const long i = row0 + row;
        act[row * ldw + col] = col < cl ? __fsub_rn(a.last[i * cl + col], pool[col]) : a.skip[i * cs + (col - cl)];
    }
    __syncthreads();
    const float *ap = act + rl * ldw + 4 * h;
    #pragma unroll 1
    for (int L = 0; L < a.l.n_layers; ++L) {
        const int G = a.l.kpad[L] >> 3, nt = a.l.npad[L] >> 5, n = a.l.nout[L];
        const float4 *wl = reinterpret_cast<const float4 *>(a.l.packed + a.l.woff[L]);
        const float *bias = a.l.packed + a.l.woff[L] + (long)a.l.kpad[L] * a.l.npad[L];
        pn_f32x16 acc[PN_HEAD_U];
        if (L < a.l.n_layers - 1) {
            const float *scale = a.bn + a.bnoff[L] + (long)p0 * n, *shift = scale + (long)PN_CELL_ROWS * n;
            pn_gemm<PN_HEAD_U, PN_HEAD_WAVES>(ap, wl, G, nt, 0, w, lane, acc);
            __syncthreads();                                             // every wavefront has read the layer's input
#pragma unroll
            for (int u = 0; u < PN_HEAD_U; ++u) {
                const int t = w + PN_HEAD_WAVES * u;
                if (t < nt) {
                    const int col = 32 * t + rl;                         // hidden: n is a multiple of 32
                    const float bv = bias[col];
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int rr = pn_acc_row(q, h);
                        float v = __fadd_rn(acc[u][q], bv);
                        v = __fadd_rn(__fmul_rn(v, scale[rr * n + col]), shift[rr * n + col]);
                        act[rr * ldw + col] = v > 0.f ? v : 0.f;
                    }
                }
            }
            __syncthreads();
        } else {
            #pragma unroll 1
            for (int t0 = 0; t0 < nt; t0 += PN_HEAD_WAVES * PN_HEAD_U) {
                pn_gemm<PN_HEAD_U, PN_HEAD_WAVES>(ap, wl, G, nt, t0, w, lane, acc);
#pragma unroll
                for (int u = 0; u < PN_HEAD_U; ++u) {
                    const int t = t0 + w + PN_HEAD_WAVES * u;
                    const int col = 32 * t + rl;
                    if (t < nt && col < n) {
                        const float bv = bias[col];
#pragma unroll
                        for (int q = 0; q < 16; ++q) a.out[(row0 + pn_acc_row(q, h)) * n + col] = __fadd_rn(acc[u][q], bv);
                    }
                }
            }
        }
    }
}

static bool pn_layer_ok(int k, int n) { return k >= 1 && k <= PN_MAX_K && n >= 1 && n <= PN_MAX_N; }

// The layer table of a stack of n_layers layers, k0 inputs, outputs widths[0 ..].  The caller has checked the widths.
static void pn_layers(int k0, int n_layers, const int32_t *widths, PnLayers *l) {
    long off = 0;
    int wide = lrg_mlp_up32(k0), k = k0;
    for (int L = 0; L < n_layers; ++L) {
        const int n = widths[L];
        l->kpad[L] = lrg_mlp_up32(k); l->nout[L] = n; l->npad[L] = lrg_mlp_up32(n); l->woff[L] = off;
        off += (long)l->kpad[L] * l->npad[L] + l->npad[L];
        if (L < n_layers - 1 && l->npad[L] > wide) wide = l->npad[L];   // the last layer's rows never return to LDS
        k = n;
    }
    l->n_layers = n_layers; l->ldw = wide + 4;
}

template <typename Kernel, typename Args>
static int pn_launch(Kernel kern, int threads, bool *attr_done, const Args &a, long tiles, hipStream_t st) {
    const int dev = lrg_current_device();
    if (!attr_done[dev]) {
        LRG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          PN_ROWS * (PN_MAX_CONCAT + 4) * 4));
        attr_done[dev] = true;
    }
    const size_t lds = (size_t)PN_ROWS * a.l.ldw * sizeof(float);
    hipLaunchKernelGGL(kern, dim3((unsigned)tiles), dim3(threads), lds, st, a);
    LRG_LAUNCH_CHECK();
    return 0;
}

static bool pn_conv_widths_ok(int n_conv, const int32_t *widths) {
    if (n_conv < PN_MIN_CONV || n_conv > PN_MAX_CONV || !widths) return false;
    for (int i = 0; i < n_conv; ++i)
        if (widths[i] < 32 || widths[i] > PN_MAX_CONV_WIDTH || (widths[i] & 31)) return false;
    return true;
}

extern "C" {

size_t lrg_pointnet_packed_floats(int k, int n) {
    if (!pn_layer_ok(k, n)) return 0;
    return lrg_mlp_packed_floats(k, n);
}

int lrg_pointnet_pack_layer(int k, int n, const float *w, const float *bias, float *packed, void *stream) {
    if (!pn_layer_ok(k, n)) return LRG_EINVAL - 40;
    if (!w || !bias || !packed || ((uintptr_t)packed & 15)) return LRG_EINVAL - 40;
    return lrg_mlp_pack_launch(k, n, w, bias, packed, (hipStream_t)stream);
}

int lrg_pointnet_features(int cells, int n_conv, const int32_t *widths, const float *x, const float *packed, float *skip, float *last,
                          float *pooled, void *stream) {
    if (cells < 0 || cells > PN_MAX_CELLS) return LRG_EINVAL - 41;
    if (!pn_conv_widths_ok(n_conv, widths)) return LRG_EINVAL - 42;
    if (cells == 0) return 0;
    if (!x || !packed || !skip || !pooled || ((uintptr_t)packed & 15)) return LRG_EINVAL - 43;
    PnFeatArgs a = {};
    pn_layers(PN_IN, n_conv, widths, &a.l);
    a.l.packed = packed; a.x = x; a.skip = skip; a.last = last; a.pooled = reinterpret_cast<int *>(pooled);
    hipStream_t st = (hipStream_t)stream;
    LRG_HIP_CHECK(hipMemsetAsync(pooled, 0, (size_t)cells * widths[n_conv - 1] * sizeof(float), st));   // +0.0f: the identity of the maximum after ReLU
    bool wide = false;                                                   // a hidden layer of more than 512 columns: eight tiles per wavefront
    for (int i = 0; i < n_conv - 1; ++i) wide = wide || widths[i] > 512;
    static bool attr_done[2][LRG_MAX_DEVICES] = {};
    if (wide) return pn_launch(pn_features_kernel<8>, PN_THREADS, attr_done[1], a, (long)cells * PN_CELL_TILES, st);
    return pn_launch(pn_features_kernel<4>, PN_THREADS, attr_done[0], a, (long)cells * PN_CELL_TILES, st);
}

int lrg_pointnet_head(int cells, int c_last, int c_skip, const float *last, const float *skip, const float *pooled, int n_fc,
                      const int32_t *widths, const float *packed, const float *bn, float *out, void *stream) {
    if (cells < 0 || cells > PN_MAX_CELLS) return LRG_EINVAL - 44;
    if (c_last < 32 || c_last > PN_MAX_CONV_WIDTH || (c_last & 31) || c_skip < 32 || c_skip > PN_MAX_CONV_WIDTH || (c_skip & 31) ||
        c_last + c_skip > PN_MAX_CONCAT) return LRG_EINVAL - 45;
    if (n_fc < PN_MIN_FC || n_fc > PN_MAX_FC || !widths) return LRG_EINVAL - 46;
    for (int i = 0; i < n_fc - 1; ++i)
        if (widths[i] < 32 || widths[i] > PN_MAX_FC_WIDTH || (widths[i] & 31)) return LRG_EINVAL - 47;
    if (widths[n_fc - 1] < 1 || widths[n_fc - 1] > PN_MAX_N) return LRG_EINVAL - 47;
    if (cells == 0) return 0;
    if (!last || !skip || !pooled || !packed || !bn || !out || ((uintptr_t)packed & 15)) return LRG_EINVAL - 48;
    PnHeadArgs a = {};
    pn_layers(c_last + c_skip, n_fc, widths, &a.l);
    a.l.packed = packed; a.last = last; a.skip = skip; a.pooled = pooled; a.bn = bn; a.out = out; a.c_last = c_last; a.c_skip = c_skip;
    long off = 0;
    for (int i = 0; i < n_fc - 1; ++i) { a.bnoff[i] = off; off += 2L * PN_CELL_ROWS * widths[i]; }
    static bool attr_done[LRG_MAX_DEVICES] = {};
    return pn_launch(pn_head_kernel, PN_HEAD_THREADS, attr_done, a, (long)cells * PN_CELL_TILES, (hipStream_t)stream);
}

}  // extern "C"
