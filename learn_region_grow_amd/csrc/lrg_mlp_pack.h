// The packed image of one layer x W + bias for the 32-row MFMA tiles of lrg_pointnet2.hip and lrg_pointnet.hip.
//
// packed layer: [npad / 32 tiles][kpad / 8 groups][64 lanes] float4, then bias [npad].  Component q of lane l of group g of tile t is
// W[8 g + 4 (l >> 5) + q][32 t + (l & 31)] (zero outside [k, n)): the k-step the lane's half feeds to the q-th MFMA of the group.
#pragma once
#include "lrg_common.h"

#define LRG_MLP_PACK_THREADS 256

static inline int lrg_mlp_up32(int v) { return (v + 31) & ~31; }

static __global__ __launch_bounds__(LRG_MLP_PACK_THREADS) void lrg_mlp_pack_kernel(const float *w, const float *bias, int k, int n, int kpad, int npad,
                                                                                   float *out) {
    const long x = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long nw = (long)kpad * npad;
    if (x >= nw + npad) return;
    float v = 0.f;
    if (x < nw) {
        const int q = (int)(x & 3), l = (int)((x >> 2) & 63);
        const long gt = x >> 8;
        const int G = kpad >> 3, g = (int)(gt % G), t = (int)(gt / G);
        const int kk = 8 * g + 4 * (l >> 5) + q, col = 32 * t + (l & 31);
        if (kk < k && col < n) v = w[(long)kk * n + col];
    } else {
        const int col = (int)(x - nw);
        if (col < n) v = bias[col];
    }
    out[x] = v;
}

static inline size_t lrg_mlp_packed_floats(int k, int n) { return (size_t)lrg_mlp_up32(k) * lrg_mlp_up32(n) + lrg_mlp_up32(n); }

// The caller has checked k, n and the pointers.
static inline int lrg_mlp_pack_launch(int k, int n, const float *w, const float *bias, float *packed, hipStream_t st) {
    const long total = (long)lrg_mlp_packed_floats(k, n);
    hipLaunchKernelGGL(lrg_mlp_pack_kernel, dim3((unsigned)((total + LRG_MLP_PACK_THREADS - 1) / LRG_MLP_PACK_THREADS)), dim3(LRG_MLP_PACK_THREADS), 0, st,
                       w, bias, k, n, lrg_mlp_up32(k), lrg_mlp_up32(n), packed);
    LRG_LAUNCH_CHECK();
    return 0;
}
