// The shared MLPs of PointNet2 (train_pointnet.py:126-167, :193-202) for gfx950: the network's FLOPs.
//
// One kernel, two front ends.  A workgroup of four wavefronts owns one tile of 32 rows and carries it through up to three layers
// of x W + bias (ReLU) without leaving the CU:
//   fill     the tile's input rows go to LDS, act[32][ldw].  Grouped form (a set-abstraction level): row s of group g is
//            xyz[idx[g][s]] - new_xyz[g] (float32 subtraction) joined with points[idx[g][s]] -- the grouped tensors of
//            sample_and_group (:113-123) are never written to memory.  Row form (a feature-propagation level, the head): row i is
//            a[i] joined with b[i], the concat of :153 is never written either.  Columns up to the next multiple of 32 are zero.
//   layer    v_mfma_f32_32x32x2_f32.  The output's 32-column tiles are dealt to the wavefronts round robin (tile t to wavefront
//            t mod 4; at most 512 / 32 / 4 = 4 tiles = 64 accumulator registers per lane).  A operand: one ds_read_b128 per
//            lane per four k-steps (row stride ldw = width + 4 floats: the 16 lanes of a b128 lane group hit 16 distinct
//            4-bank sets).  B operand: the weights in operand order (lrg_pointnet2_pack_layer), one global_load_dwordx4 per lane
//            per four k-steps, fetched four groups (16 MFMAs) ahead.  The sum over k runs in one fixed order per output value,
//            whatever the launch holds besides.
//   hand on  all wavefronts meet, then bias + ReLU goes back into act in place (the accumulators held the whole layer, so one
//            buffer serves input and output) and they meet again.
//   last     grouped: bias, ReLU, the maximum over the lane's 16 rows, then over the two lane halves (no atomics); row form:
//            bias (ReLU unless relu_last == 0) straight to out.
//   keep     the training forms (KEEP; lrg_pointnet2_*_mlp_train) also store what the backward pass reads: the rows as filled
//            (grouped form) and every layer's post-ReLU output, [rows, width] unpadded.  The stores sit beside the arithmetic,
//            never in it: the last output carries the same bits with and without them.
// LDS: 32 * (max width + 4) * 4 bytes, dynamic: 131.6 KB for the widest legal input (1024), 16.9 KB for a 128-wide level, so the
// narrow levels keep several workgroups on a CU.
#include "lrg_common.h"
#include "lrg_mlp_pack.h"

#define PN2_THREADS 256
#define PN2_ROWS 32
#define PN2_MAX_LAYERS 3
#define PN2_MAX_IN 1024
#define PN2_MAX_WIDTH 512
#define PN2_LDS_MAX (PN2_ROWS * (PN2_MAX_IN + 4) * 4)

typedef float pn2_f32x16 __attribute__((ext_vector_type(16)));

struct Pn2Args {
    // grouped form
    const float *xyz, *new_xyz, *points; const int32_t *idx; int n, m, c;
    // row form
    const float *a, *b; int ca, cb; long r;
    // both
    long tiles;
    int n_layers, relu_last, ldw, k0;
    int kpad[PN2_MAX_LAYERS], nout[PN2_MAX_LAYERS], npad[PN2_MAX_LAYERS];
    long woff[PN2_MAX_LAYERS];
    const float *packed; float *out;
    // training forms only (each nullable): the filled rows [tiles * 32, k0] and the layers' post-ReLU outputs [rows, nout[L]]
    float *rows_out; float *keep[PN2_MAX_LAYERS];
};

static inline int pn2_up32(int v) { return lrg_mlp_up32(v); }

template <bool GROUPED, bool KEEP>
__global__ __launch_bounds__(PN2_THREADS) void pn2_mlp_kernel(Pn2Args a) {
    extern __shared__ __attribute__((aligned(16))) float pn2_act[];      // [32][ldw]
    __shared__ int s_j[PN2_ROWS];
    float *act = pn2_act;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, h = lane >> 5, rl = lane & 31;
    const long tile = blockIdx.x;
    const int ldw = a.ldw, k0 = a.k0, k0p = a.kpad[0];
    const long row0 = tile * PN2_ROWS;
    if (GROUPED) {
        const long bi = tile / a.m;
        if (tid < PN2_ROWS) {
            int j = a.idx[tile * PN2_ROWS + tid];
            if ((unsigned)j >= (unsigned)a.n) j = 0;                        // never an address outside the batch element
            s_j[tid] = j;
        }
        __syncthreads();
        const float *xb = a.xyz + bi * a.n * 3, *ctr = a.new_xyz + tile * 3;
        const float *pb = a.points ? a.points + bi * a.n * a.c : nullptr;
        for (int e = tid; e < PN2_ROWS * k0p; e += PN2_THREADS) {
            const int row = e / k0p, col = e - row * k0p;
            const int j = s_j[row];
            float v = 0.f;
            if (col < 3) v = __fsub_rn(xb[(long)j * 3 + col], ctr[col]);
            else if (col < k0) v = pb[(long)j * a.c + (col - 3)];
            act[row * ldw + col] = v;
            if (KEEP && a.rows_out && col < k0) a.rows_out[(row0 + row) * k0 + col] = v;
        }
    } else {
        for (int e = tid; e < PN2_ROWS * k0p; e += PN2_THREADS) {
            const int row = e / k0p, col = e - row * k0p;
            const long i = row0 + row;
            float v = 0.f;
            if (i < a.r) {
                if (col < a.ca) v = a.a[i * a.ca + col];
                else if (col < k0) v = a.b[i * a.cb + (col - a.ca)];
            }
            act[row * ldw + col] = v;
        }
    }
    __syncthreads();
    #pragma unroll 1
    for (int L = 0; L < a.n_layers; ++L) {
        const int G = a.kpad[L] >> 3, nt = a.npad[L] >> 5;               // G is a multiple of 4
        const float4 *wl = reinterpret_cast<const float4 *>(a.packed + a.woff[L]);
        const float *bias = a.packed + a.woff[L] + (long)a.kpad[L] * a.npad[L];
        const bool last = L == a.n_layers - 1;
        pn2_f32x16 acc[4];
        const float *ap = act + rl * ldw + 4 * h;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = w + 4 * u;
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[u][q] = 0.f;
            if (t < nt) {                                                // the same for every lane of the wavefront
                const float4 *wp = wl + (long)t * G * 64 + lane;
                float4 bq[4], bn[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) bq[i] = wp[i * 64];
                #pragma unroll 1
                for (int g0 = 0; g0 < G; g0 += 4) {
                    const int gn = g0 + 4 < G ? g0 + 4 : g0;             // the last round reloads its own groups (unused)
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
        if (!last) {
            __syncthreads();                                             // every wavefront has read the layer's input
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int t = w + 4 * u;
                if (t < nt) {
                    const int col = 32 * t + rl;
                    const float bv = bias[col];
                    float *kp = KEEP ? a.keep[L] : nullptr;              // hidden widths are multiples of 32: col < nout[L]
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int rr = (q & 3) + 8 * (q >> 2) + 4 * h;
                        const float v = __fadd_rn(acc[u][q], bv);
                        const float y = v > 0.f ? v : 0.f;
                        act[rr * ldw + col] = y;
                        if (KEEP && kp && (GROUPED || row0 + rr < a.r)) kp[(row0 + rr) * a.nout[L] + col] = y;
                    }
                }
            }
            __syncthreads();
        } else {
            const int n_out = a.nout[L];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int t = w + 4 * u;
                if (t < nt) {
                    const int col = 32 * t + rl;
                    const float bv = bias[col];
                    if (GROUPED) {
                        float mx = 0.f;                                  // ReLU output: the maximum is >= 0
#pragma unroll
                        for (int q = 0; q < 16; ++q) mx = fmaxf(mx, __fadd_rn(acc[u][q], bv));
                        if (KEEP && a.keep[L] && col < n_out) {
#pragma unroll
                            for (int q = 0; q < 16; ++q) {
                                const float v = __fadd_rn(acc[u][q], bv);
                                a.keep[L][(row0 + (q & 3) + 8 * (q >> 2) + 4 * h) * n_out + col] = v > 0.f ? v : 0.f;
                            }
                        }
                        mx = fmaxf(mx, __shfl_xor(mx, 32));
                        if (h == 0 && col < n_out) a.out[tile * n_out + col] = mx;
                    } else {
#pragma unroll
                        for (int q = 0; q < 16; ++q) {
                            const long i = row0 + (q & 3) + 8 * (q >> 2) + 4 * h;
                            float v = __fadd_rn(acc[u][q], bv);
                            if (a.relu_last) v = v > 0.f ? v : 0.f;
                            if (i < a.r && col < n_out) a.out[i * n_out + col] = v;
                            if (KEEP && a.keep[L] && i < a.r && col < n_out) a.keep[L][i * n_out + col] = v;
                        }
                    }
                }
            }
        }
    }
}

// The packed layer image and its kernel: lrg_mlp_pack.h (shared with lrg_pointnet.hip).
static bool pn2_layer_ok(int k, int n) { return k >= 1 && k <= PN2_MAX_IN && n >= 1 && n <= PN2_MAX_WIDTH; }

// widths[0] the input width, widths[1 ..] the layers' outputs.  Fills the layer table of `a`; every hidden width a multiple of 32.
static int pn2_layers(int n_layers, const int32_t *widths, bool last_any, Pn2Args *a) {
    if (n_layers < 1 || n_layers > PN2_MAX_LAYERS || !widths) return LRG_EINVAL - 91;
    if (widths[0] < 1 || widths[0] > PN2_MAX_IN) return LRG_EINVAL - 92;
    long off = 0;
    int wide = pn2_up32(widths[0]);
    for (int L = 0; L < n_layers; ++L) {
        const int k = widths[L], n = widths[L + 1];
        const bool last = L == n_layers - 1;
        if (n < 1 || n > PN2_MAX_WIDTH) return LRG_EINVAL - 93;
        if ((n & 31) && !(last && last_any)) return LRG_EINVAL - 94;
        a->kpad[L] = pn2_up32(k); a->nout[L] = n; a->npad[L] = pn2_up32(n); a->woff[L] = off;
        off += (long)a->kpad[L] * a->npad[L] + a->npad[L];
        if (!last && a->npad[L] > wide) wide = a->npad[L];
    }
    for (int L = n_layers; L < PN2_MAX_LAYERS; ++L) { a->kpad[L] = 0; a->nout[L] = 0; a->npad[L] = 0; a->woff[L] = 0; }
    a->n_layers = n_layers; a->k0 = widths[0]; a->ldw = wide + 4;
    return 0;
}

template <bool GROUPED, bool KEEP>
static int pn2_launch(const Pn2Args &a, hipStream_t st) {
    auto kern = pn2_mlp_kernel<GROUPED, KEEP>;
    static bool attr_done[LRG_MAX_DEVICES] = {};
    const int dev = lrg_current_device();
    if (!attr_done[dev]) {
        LRG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, PN2_LDS_MAX));
        attr_done[dev] = true;
    }
    const size_t lds = (size_t)PN2_ROWS * a.ldw * sizeof(float);
    hipLaunchKernelGGL(kern, dim3((unsigned)a.tiles), dim3(PN2_THREADS), lds, st, a);
    LRG_LAUNCH_CHECK();
    return 0;
}

// The argument checks and the launch of both grouped forms (KEEP = false: the inference form, rows and keep unused), then of both row forms.
template <bool KEEP>
static int pn2_group_mlp(int b, int n, int m, int nsample, int c, const float *xyz, const float *new_xyz, const float *points,
                         const int32_t *idx, const int32_t *widths, const float *packed, float *out, float *rows, float *const *keep,
                         void *stream) {
    if (nsample != PN2_ROWS) return LRG_EINVAL - 95;
    if (b < 0 || n < 1 || m < 0 || c < 0 || c > PN2_MAX_IN - 3) return LRG_EINVAL - 96;
    if (!widths) return LRG_EINVAL - 91;
    Pn2Args a = {};
    const int32_t w4[4] = {3 + c, widths[0], widths[1], widths[2]};
    int rc = pn2_layers(3, w4, false, &a);
    if (rc) return rc;
    const long groups = (long)b * m;
    if (groups == 0) return 0;
    if (groups > (1L << 30)) return LRG_EINVAL - 96;
    if (!xyz || !new_xyz || !idx || !packed || !out || (c > 0 && !points) || ((uintptr_t)packed & 15)) return LRG_EINVAL - 97;
    a.xyz = xyz; a.new_xyz = new_xyz; a.points = c > 0 ? points : nullptr; a.idx = idx; a.n = n; a.m = m; a.c = c;
    a.tiles = groups; a.relu_last = 1; a.packed = packed; a.out = out;
    if (KEEP) { a.rows_out = rows; for (int L = 0; L < 3; ++L) a.keep[L] = keep[L]; }
    return pn2_launch<true, KEEP>(a, (hipStream_t)stream);
}

template <bool KEEP>
static int pn2_row_mlp(long r, int ca, int cb, const float *rows_a, const float *rows_b, int n_layers, const int32_t *widths,
                       int relu_last, const float *packed, float *out, float *const *keep, void *stream) {
    if (r < 0 || r > (1L << 35) || ca < 1 || cb < 0 || ca > PN2_MAX_IN || cb > PN2_MAX_IN || ca + cb > PN2_MAX_IN) return LRG_EINVAL - 98;
    if (n_layers < 1 || n_layers > PN2_MAX_LAYERS || !widths || (relu_last != 0 && relu_last != 1)) return LRG_EINVAL - 91;
    Pn2Args a = {};
    int32_t w4[4] = {ca + cb, 0, 0, 0};
    for (int L = 0; L < n_layers; ++L) w4[L + 1] = widths[L];
    int rc = pn2_layers(n_layers, w4, true, &a);
    if (rc) return rc;
    if (r == 0) return 0;
    if (!rows_a || (cb > 0 && !rows_b) || !packed || !out || ((uintptr_t)packed & 15)) return LRG_EINVAL - 97;
    a.a = rows_a; a.b = cb > 0 ? rows_b : nullptr; a.ca = ca; a.cb = cb; a.r = r;
    a.tiles = (r + PN2_ROWS - 1) / PN2_ROWS; a.relu_last = relu_last; a.packed = packed; a.out = out;
    if (KEEP) for (int L = 0; L < n_layers; ++L) a.keep[L] = keep[L];
    return pn2_launch<false, KEEP>(a, (hipStream_t)stream);
}

extern "C" {

size_t lrg_pointnet2_packed_floats(int k, int n) {
    if (!pn2_layer_ok(k, n)) return 0;
    return (size_t)pn2_up32(k) * pn2_up32(n) + pn2_up32(n);
}

int lrg_pointnet2_pack_layer(int k, int n, const float *w, const float *bias, float *packed, void *stream) {
    if (!pn2_layer_ok(k, n)) return LRG_EINVAL - 90;
    if (!w || !bias || !packed || ((uintptr_t)packed & 15)) return LRG_EINVAL - 90;
    return lrg_mlp_pack_launch(k, n, w, bias, packed, (hipStream_t)stream);
}

int lrg_pointnet2_group_mlp(int b, int n, int m, int nsample, int c, const float *xyz, const float *new_xyz, const float *points,
                            const int32_t *idx, const int32_t *widths, const float *packed, float *out, void *stream) {
    return pn2_group_mlp<false>(b, n, m, nsample, c, xyz, new_xyz, points, idx, widths, packed, out, nullptr, nullptr, stream);
}

int lrg_pointnet2_row_mlp(long r, int ca, int cb, const float *rows_a, const float *rows_b, int n_layers, const int32_t *widths,
                          int relu_last, const float *packed, float *out, void *stream) {
    return pn2_row_mlp<false>(r, ca, cb, rows_a, rows_b, n_layers, widths, relu_last, packed, out, nullptr, stream);
}

int lrg_pointnet2_group_mlp_train(int b, int n, int m, int nsample, int c, const float *xyz, const float *new_xyz, const float *points,
                                  const int32_t *idx, const int32_t *widths, const float *packed, float *out, float *rows, float *keep0,
                                  float *keep1, float *keep2, void *stream) {
    float *const keep[3] = {keep0, keep1, keep2};
    return pn2_group_mlp<true>(b, n, m, nsample, c, xyz, new_xyz, points, idx, widths, packed, out, rows, keep, stream);
}

int lrg_pointnet2_row_mlp_train(long r, int ca, int cb, const float *rows_a, const float *rows_b, int n_layers, const int32_t *widths,
                                int relu_last, const float *packed, float *out, float *keep0, float *keep1, float *keep2, void *stream) {
    float *const keep[3] = {keep0, keep1, keep2};
    return pn2_row_mlp<true>(r, ca, cb, rows_a, rows_b, n_layers, widths, relu_last, packed, out, keep, stream);
}

}  // extern "C"
