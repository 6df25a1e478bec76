// The exclusive scan of an int32 array that preprocessing, the baselines and MCPNet's candidate lists share (lrg_exscan_i32, declared
// in lrg_common.h): block sums, one block that scans the sums, then every block again with its base.
#include "lrg_common.h"

#define SCAN_THREADS 256
#define SCAN_ITEMS (LRG_SCAN_BLOCK / SCAN_THREADS)

// exclusive scan of one value per thread over the block; *total = the block's sum
__device__ __forceinline__ int scan_block_exscan(int v, int *sh, int *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int inc = lrg_wave_incl_scan_i32(v);
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    int base = 0, tot = 0;
    for (int k = 0; k < SCAN_THREADS / 64; ++k) {
        if (k < w) base += sh[k];
        tot += sh[k];
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

__global__ __launch_bounds__(SCAN_THREADS) void scan_sums_kernel(const int32_t *x, long n, int32_t *bsum) {
    __shared__ int sh[SCAN_THREADS / 64];
    const long base = ((long)blockIdx.x * SCAN_THREADS + threadIdx.x) * SCAN_ITEMS;
    int s = 0;
    for (int k = 0; k < SCAN_ITEMS; ++k) s += base + k < n ? x[base + k] : 0;
    int tot;
    scan_block_exscan(s, sh, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

__global__ __launch_bounds__(SCAN_THREADS) void scan_top_kernel(int32_t *bsum, int nb) {   // one block; bsum[nb] = total
    __shared__ int sh[SCAN_THREADS / 64];
    int carry = 0;
    for (int b0 = 0; b0 < nb; b0 += SCAN_THREADS) {
        const int i = b0 + threadIdx.x;
        const int v = i < nb ? bsum[i] : 0;
        int tot;
        const int ex = scan_block_exscan(v, sh, &tot);
        if (i < nb) bsum[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) bsum[nb] = carry;
}

__global__ __launch_bounds__(SCAN_THREADS) void scan_apply_kernel(const int32_t *x, long n, const int32_t *bsum, int32_t *out) {
    __shared__ int sh[SCAN_THREADS / 64];
    const long base = ((long)blockIdx.x * SCAN_THREADS + threadIdx.x) * SCAN_ITEMS;
    int v[SCAN_ITEMS], s = 0;
    for (int k = 0; k < SCAN_ITEMS; ++k) { v[k] = base + k < n ? x[base + k] : 0; s += v[k]; }
    int tot;
    int run = bsum[blockIdx.x] + scan_block_exscan(s, sh, &tot);
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        if (base + k < n) out[base + k] = run;
        run += v[k];
    }
}

extern "C" int lrg_exscan_i32(const int32_t *x, long n, int32_t *bsum, int32_t *out, void *stream) {
    if (n == 0) return 0;
    if (n < 0 || lrg_scan_blocks(n) > INT_MAX || !x || !bsum || !out) return LRG_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int nb = (int)lrg_scan_blocks(n);
    hipLaunchKernelGGL(scan_sums_kernel, dim3(nb), dim3(SCAN_THREADS), 0, st, x, n, bsum);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, bsum, nb);
    hipLaunchKernelGGL(scan_apply_kernel, dim3(nb), dim3(SCAN_THREADS), 0, st, x, n, bsum, out);
    LRG_LAUNCH_CHECK();
    return 0;
}
