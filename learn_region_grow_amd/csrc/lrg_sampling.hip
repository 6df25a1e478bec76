// tf_ops/sampling and tf_ops/3d_interpolation replacements for gfx950 (reference: tf_ops/sampling/tf_sampling_g.cu,
// tf_ops/3d_interpolation/tf_interpolate.cpp -- the latter runs on the CPU only there).
//
// Farthest point sampling (farthestpointsamplingKernel, tf_sampling_g.cu:105-170).  The reference scans with 512 threads
// in stride order, keeping a thread's first maximum (strict >), then reduces with a tree that keeps the LEFT entry on
// equality.  Among equal maxima it therefore picks the point with the smallest (k mod 512, k).  Here every candidate
// carries the 64-bit key  (float bits of its running minimum) << 32 | ~rank,  rank = (k mod 512) * ceil(n/512) + k / 512,
// and the largest key wins: non-negative floats order like their bits, and a smaller rank is a larger ~rank.  With this
// rule duplicate points and m > n give the reference's indices (once every minimum is 0, index 0 repeats).
//
// One workgroup of 1024 threads per batch element; thread t owns the points t, t + 1024, ... (all of one class k mod 512,
// in increasing k, so a thread's own strict > scan already follows the tie order).  Two variants:
//   - registers: coordinates and running minima of up to P points per thread in VGPRs, P in {1, 4, 8, 16} (n <= 16384).
//     (32 points per thread would be 4 x 32 x 1024 x 4 B = 512 KB: the whole register file of a CU, before any temporaries.)
//   - streaming: larger n; the running minima live in a caller-supplied temp of b * n floats, coordinates come from L2.
// Per step: each wave finds its maximum by DPP and its tie winner by a ballot, the winning lane writes (key, coordinates, index) to an LDS slot,
// one barrier, and every thread reduces the 16 slots itself.  The slots are double-buffered, so no second barrier.
#include "lrg_common.h"

#define LRG_FPS_THREADS 1024
#define LRG_FPS_WAVES (LRG_FPS_THREADS / 64)
#define LRG_FPS_MAX_REG_POINTS (16 * LRG_FPS_THREADS)

__device__ __forceinline__ float lrg_sqdist3(float x1, float y1, float z1, float x2, float y2, float z2) {
    const float dx = __fsub_rn(x2, x1), dy = __fsub_rn(y2, y1), dz = __fsub_rn(z2, z1);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// Wave maximum by DPP within each row of 16 lanes (row_shr 1, 2, 4, 8: lane 15 of a row holds the row's maximum), then the four
// rows' lane 15 read as scalars.  The result is wave-uniform.
__device__ __forceinline__ int lrg_wave_max_i32(int v) {
    v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x111, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x112, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x114, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(INT_MIN, v, 0x118, 0xf, 0xf, false));
    return max(max(__builtin_amdgcn_readlane(v, 15), __builtin_amdgcn_readlane(v, 31)),
               max(__builtin_amdgcn_readlane(v, 47), __builtin_amdgcn_readlane(v, 63)));
}

// P > 0: registers, P points per thread.  P == 0: streaming through temp.
template <int P>
__global__ __launch_bounds__(LRG_FPS_THREADS) void lrg_fps_kernel(int n, int m, const float *__restrict__ inp, float *__restrict__ temp,
                                                                  int *__restrict__ out) {
    __shared__ unsigned long long skey[2][LRG_FPS_WAVES];
    __shared__ int4 sinfo[2][LRG_FPS_WAVES];
    const int t = threadIdx.x, w = t >> 6;
    const float *p = inp + (size_t)blockIdx.x * n * 3;
    int *o = out + (size_t)blockIdx.x * m;
    float *tmp = P == 0 ? temp + (size_t)blockIdx.x * n : nullptr;
    const unsigned Q = ((unsigned)n + 511u) >> 9;
    constexpr int PR = P > 0 ? P : 1;
    float px[PR], py[PR], pz[PR], pd[PR];
    if (P > 0) {
#pragma unroll
        for (int j = 0; j < PR; ++j) {
            const int k = t + LRG_FPS_THREADS * j;
            const bool ok = k < n;
            px[j] = ok ? p[k * 3 + 0] : 0.f;
            py[j] = ok ? p[k * 3 + 1] : 0.f;
            pz[j] = ok ? p[k * 3 + 2] : 0.f;
            pd[j] = ok ? 1e38f : -2.f;          // padding: its minimum stays -2, never above the scan's starting -1
        }
    } else {
        for (int k = t; k < n; k += LRG_FPS_THREADS) tmp[k] = 1e38f;
    }
    if (t < 2 * LRG_FPS_WAVES) skey[t / LRG_FPS_WAVES][t % LRG_FPS_WAVES] = 0ull;     // a wave without points never writes its slot
    float x1 = p[0], y1 = p[1], z1 = p[2];
    if (t == 0) o[0] = 0;
    __syncthreads();
    for (int s = 1; s < m; ++s) {
        float best = -1.f, bx = 0.f, by = 0.f, bz = 0.f;
        int bk = 0;
        if (P > 0) {
#pragma unroll
            for (int j = 0; j < PR; ++j) {
                const float d2 = fminf(lrg_sqdist3(x1, y1, z1, px[j], py[j], pz[j]), pd[j]);
                pd[j] = d2;
                if (d2 > best) { best = d2; bk = j; bx = px[j]; by = py[j]; bz = pz[j]; }
            }
            bk = t + LRG_FPS_THREADS * bk;
        } else {
#pragma unroll 4
            for (int k = t; k < n; k += LRG_FPS_THREADS) {
                const float x2 = p[k * 3 + 0], y2 = p[k * 3 + 1], z2 = p[k * 3 + 2], td = tmp[k];
                const float d2 = fminf(lrg_sqdist3(x1, y1, z1, x2, y2, z2), td);
                if (d2 != td) tmp[k] = d2;
                if (d2 > best) { best = d2; bk = k; bx = x2; by = y2; bz = z2; }
            }
        }
        // Within a wave the lanes' classes (k mod 512) increase with the lane, so among equal maxima the lowest lane is the tie
        // rule's choice: a max of the float bits (non-negative floats order like signed ints; -1 stays negative) and a ballot.
        const int bits = __float_as_int(best);
        const int wmax = lrg_wave_max_i32(bits);
        const int wl = (int)__ffsll((long long)__ballot(bits == wmax)) - 1;
        const int buf = s & 1;
        if (wmax >= 0 && lrg_lane() == wl) {   // a wave without points (wmax < 0) leaves its slot at key 0
            const unsigned rank = ((unsigned)bk & 511u) * Q + ((unsigned)bk >> 9);
            skey[buf][w] = ((unsigned long long)(unsigned)bits << 32) | (unsigned long long)(~rank);
            sinfo[buf][w] = make_int4(__float_as_int(bx), __float_as_int(by), __float_as_int(bz), bk);
        }
        __syncthreads();
        unsigned long long kbest = skey[buf][0];
        int wb = 0;
#pragma unroll
        for (int i = 1; i < LRG_FPS_WAVES; ++i) {
            const unsigned long long ki = skey[buf][i];
            if (ki > kbest) { kbest = ki; wb = i; }
        }
        const int4 win = sinfo[buf][wb];
        x1 = __int_as_float(win.x); y1 = __int_as_float(win.y); z1 = __int_as_float(win.z);
        if (t == 0) o[s] = win.w;
    }
}

// ---- gather_point / its gradient (gatherpointKernel, scatteraddpointKernel: tf_sampling_g.cu:172-192).  An index outside
// [0, n) gathers zeros and scatters nothing (the reference reads and writes out of bounds there). ----
template <typename I>
__global__ void lrg_gather_point_kernel(I total, int n, int m, const float *__restrict__ inp, const int *__restrict__ idx, float *__restrict__ out) {
    const I e = (I)blockIdx.x * blockDim.x + threadIdx.x;          // one (batch, row, coordinate)
    if (e >= total) return;
    const I q = e / 3;
    const int d = (int)(e - q * 3);
    const I bi = q / m;
    const int a = idx[q];
    out[e] = (a >= 0 && a < n) ? inp[((long)bi * n + a) * 3 + d] : 0.f;
}

template <typename I>
__global__ void lrg_scatter_add_point_kernel(I total, int n, int m, const float *__restrict__ out_g, const int *__restrict__ idx, float *__restrict__ inp_g) {
    const I e = (I)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const I q = e / 3;
    const int d = (int)(e - q * 3);
    const I bi = q / m;
    const int a = idx[q];
    if (a >= 0 && a < n) atomicAdd(&inp_g[((long)bi * n + a) * 3 + d], out_g[e]);
}

// ---- prob_sample (probsampleLauncher, tf_sampling_g.cu:194-197): inclusive cumsum per row, then binarysearchKernel (:90-104).
// Summation order of the cdf: the row is cut into 1024 contiguous chunks of ceil(n/1024) entries; a thread sums its chunk
// left to right, the chunk totals are scanned (Hillis-Steele within each wave, then the wave totals the same way), and the
// thread re-walks its chunk left to right from its exclusive prefix.  Integer-valued weights below 2^24 are exact. ----
__global__ __launch_bounds__(1024) void lrg_cumsum_kernel(int n, const float *__restrict__ inp, float *__restrict__ cdf) {
    __shared__ float wtot[16];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const float *x = inp + (size_t)blockIdx.x * n;
    float *y = cdf + (size_t)blockIdx.x * n;
    const int chunk = (n + 1023) / 1024;
    const int k0 = min(n, t * chunk), k1 = min(n, k0 + chunk);
    float s = 0.f;
    for (int k = k0; k < k1; ++k) s = __fadd_rn(s, x[k]);
    float v = s;                                        // inclusive scan of chunk totals within the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float u = __shfl_up(v, off);
        if (lane >= off) v = __fadd_rn(u, v);
    }
    if (lane == 63) wtot[w] = v;
    __syncthreads();
    float wpre = 0.f;                                   // exclusive prefix of the wave totals
    for (int i = 0; i < w; ++i) wpre = __fadd_rn(wpre, wtot[i]);
    const float vprev = __shfl_up(v, 1);               // the previous lane's inclusive total
    float run = lane == 0 ? wpre : __fadd_rn(wpre, vprev);   // exclusive prefix of this chunk
    for (int k = k0; k < k1; ++k) { run = __fadd_rn(run, x[k]); y[k] = run; }
}

__global__ void lrg_binary_search_kernel(int b, int n, int m, const float *__restrict__ cdf, const float *__restrict__ query, int *__restrict__ result) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long)b * m) return;
    const long i = e / m;
    const float *row = cdf + i * n;
    int base = 1;
    while (base < n) base <<= 1;
    const float q = __fmul_rn(query[e], row[n - 1]);
    int r = n - 1;
    for (int k = base; k >= 1; k >>= 1)
        if (r >= k && row[r - k] >= q) r -= k;
    result[e] = r;
}

// ---- three_nn (threenn_cpu, tf_interpolate.cpp:60-104), bit for bit: one query per lane, the known points staged through LDS
// in tiles.  The reference widens the fp32 distance to double before comparing; fp32 compares are the same.  Cascade by
// strict <, so the first index wins ties; missing slots (m < 3) keep index 0 and (float)1e40 = inf. ----
#define LRG_NN_THREADS 256
#define LRG_NN_TILE 1024

__device__ __forceinline__ void lrg_three_nn_query(int m, const float *__restrict__ p2, float (*tile)[3], float x1, float y1, float z1, bool live,
                                                   float bd[3], int bi[3]) {
    bd[0] = bd[1] = bd[2] = __int_as_float(0x7f800000);
    bi[0] = bi[1] = bi[2] = 0;
    for (int k0 = 0; k0 < m; k0 += LRG_NN_TILE) {
        const int cnt = min(LRG_NN_TILE, m - k0);
        __syncthreads();
        for (int e = threadIdx.x; e < cnt * 3; e += LRG_NN_THREADS) (&tile[0][0])[e] = p2[(size_t)k0 * 3 + e];
        __syncthreads();
        if (!live) continue;
        for (int kk = 0; kk < cnt; ++kk) {
            const float d = lrg_sqdist3(x1, y1, z1, tile[kk][0], tile[kk][1], tile[kk][2]);
            const int k = k0 + kk;
            if (d < bd[0]) {
                bd[2] = bd[1]; bi[2] = bi[1]; bd[1] = bd[0]; bi[1] = bi[0]; bd[0] = d; bi[0] = k;
            } else if (d < bd[1]) {
                bd[2] = bd[1]; bi[2] = bi[1]; bd[1] = d; bi[1] = k;
            } else if (d < bd[2]) {
                bd[2] = d; bi[2] = k;
            }
        }
    }
}

__global__ __launch_bounds__(LRG_NN_THREADS) void lrg_three_nn_kernel(int n, int m, int qblocks, const float *__restrict__ xyz1, const float *__restrict__ xyz2,
                                                                       float *__restrict__ dist, int *__restrict__ idx) {
    __shared__ float tile[LRG_NN_TILE][3];
    const long bi = blockIdx.x / qblocks;
    const int j = (blockIdx.x - (int)(bi * qblocks)) * LRG_NN_THREADS + threadIdx.x;
    const bool live = j < n;
    const float *q = xyz1 + (bi * n + (live ? j : 0)) * 3;
    float bd[3];
    int bx[3];
    lrg_three_nn_query(m, xyz2 + bi * m * 3, tile, q[0], q[1], q[2], live, bd, bx);
    if (!live) return;
    const long o = (bi * n + j) * 3;
    for (int i = 0; i < 3; ++i) { dist[o + i] = bd[i]; idx[o + i] = bx[i]; }
}

// ---- three_interpolate (threeinterpolate_cpu, :107-128): out = p[i1] w1 + p[i2] w2 + p[i3] w3, left to right, no FMA.  An index
// outside [0, m) contributes 0 * w. ----
__device__ __forceinline__ float lrg_interp3(const float *pts, int m, int c, int l, const int i[3], const float w[3]) {
    float v[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) v[u] = (i[u] >= 0 && i[u] < m) ? pts[(long)i[u] * c + l] : 0.f;
    return __fadd_rn(__fadd_rn(__fmul_rn(v[0], w[0]), __fmul_rn(v[1], w[1])), __fmul_rn(v[2], w[2]));
}

template <typename I>
__global__ void lrg_three_interpolate_kernel(I total, int m, int c, int n, const float *__restrict__ points, const int *__restrict__ idx,
                                             const float *__restrict__ weight, float *__restrict__ out) {
    const I e = (I)blockIdx.x * blockDim.x + threadIdx.x;         // one (batch, query, channel)
    if (e >= total) return;
    const I q = e / c;
    const int l = (int)(e - q * c);
    const I bi = q / n;
    const int i[3] = {idx[q * 3 + 0], idx[q * 3 + 1], idx[q * 3 + 2]};
    const float w[3] = {weight[q * 3 + 0], weight[q * 3 + 1], weight[q * 3 + 2]};
    out[e] = lrg_interp3(points + (long)bi * m * c, m, c, l, i, w);
}

// (threeinterpolate_grad_cpu, :131-155) scattered with fp32 atomics into a grad_points the caller zeroed
template <typename I>
__global__ void lrg_three_interpolate_grad_kernel(I total, int n, int c, int m, const float *__restrict__ grad_out, const int *__restrict__ idx,
                                                  const float *__restrict__ weight, float *__restrict__ grad_points) {
    const I e = (I)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const I q = e / c;
    const int l = (int)(e - q * c);
    const I bi = q / n;
    const float g = grad_out[e];
    float *gp = grad_points + (long)bi * m * c;
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int a = idx[q * 3 + u];
        if (a >= 0 && a < m) atomicAdd(&gp[(long)a * c + l], __fmul_rn(g, weight[q * 3 + u]));
    }
}

// ---- three_nn + inverse-distance weights + three_interpolate in one launch (pointnet_fp_module, train_pointnet.py:145-150):
// inv_i = 1 / max(d_i, 1e-10f) (correctly rounded), norm = (inv_0 + inv_1) + inv_2, w_i = inv_i / norm.  A block's 256
// queries keep their indices and weights in LDS, then interpolate channel-fastest so row reads and output writes coalesce. ----
__global__ __launch_bounds__(LRG_NN_THREADS) void lrg_three_nn_interpolate_kernel(int n, int m, int c, int qblocks, const float *__restrict__ xyz1,
                                                                                   const float *__restrict__ xyz2, const float *__restrict__ points,
                                                                                   float *__restrict__ dist, int *__restrict__ idx, float *__restrict__ weight,
                                                                                   float *__restrict__ out) {
    __shared__ float tile[LRG_NN_TILE][3];
    __shared__ int sidx[LRG_NN_THREADS][3];
    __shared__ float sw[LRG_NN_THREADS][3];
    const long bi = blockIdx.x / qblocks;
    const int j0 = (blockIdx.x - (int)(bi * qblocks)) * LRG_NN_THREADS;
    const int j = j0 + threadIdx.x;
    const bool live = j < n;
    const float *q = xyz1 + (bi * n + (live ? j : 0)) * 3;
    float bd[3];
    int bx[3];
    lrg_three_nn_query(m, xyz2 + bi * m * 3, tile, q[0], q[1], q[2], live, bd, bx);
    if (live) {
        float inv[3];
#pragma unroll
        for (int u = 0; u < 3; ++u) inv[u] = __fdiv_rn(1.0f, fmaxf(bd[u], 1e-10f));
        const float norm = __fadd_rn(__fadd_rn(inv[0], inv[1]), inv[2]);
        const long o = (bi * n + j) * 3;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            sidx[threadIdx.x][u] = bx[u];
            sw[threadIdx.x][u] = __fdiv_rn(inv[u], norm);
            if (dist) dist[o + u] = bd[u];
            if (idx) idx[o + u] = bx[u];
            if (weight) weight[o + u] = sw[threadIdx.x][u];
        }
    }
    __syncthreads();
    const int rows = min(LRG_NN_THREADS, n - j0);
    const float *pts = points + bi * m * c;
    float *ob = out + ((long)bi * n + j0) * c;
    for (unsigned e = threadIdx.x; e < (unsigned)(rows * c); e += LRG_NN_THREADS) {
        const int r = (int)(e / (unsigned)c), l = (int)(e - (unsigned)r * c);
        const int i[3] = {sidx[r][0], sidx[r][1], sidx[r][2]};
        const float w[3] = {sw[r][0], sw[r][1], sw[r][2]};
        ob[e] = lrg_interp3(pts, m, c, l, i, w);
    }
}

static inline unsigned lrg_blocks(long total, int threads) { return (unsigned)((total + threads - 1) / threads); }

extern "C" {

int lrg_farthest_point_sample(int b, int n, int m, const float *inp, float *temp, int *out, void *stream) {
    if (b < 0 || n < 0) return LRG_EINVAL - 1;
    if (m <= 0 || b == 0) return 0;
    if (n == 0 || !inp || !out) return LRG_EINVAL - 1;
    if ((long)n * 3 >= 0x7fffffffL) return LRG_EINVAL - 2;
    hipStream_t s = (hipStream_t)stream;
    const dim3 g((unsigned)b), blk(LRG_FPS_THREADS);
    if (n <= LRG_FPS_THREADS) hipLaunchKernelGGL(lrg_fps_kernel<1>, g, blk, 0, s, n, m, inp, nullptr, out);
    else if (n <= 4 * LRG_FPS_THREADS) hipLaunchKernelGGL(lrg_fps_kernel<4>, g, blk, 0, s, n, m, inp, nullptr, out);
    else if (n <= 8 * LRG_FPS_THREADS) hipLaunchKernelGGL(lrg_fps_kernel<8>, g, blk, 0, s, n, m, inp, nullptr, out);
    else if (n <= LRG_FPS_MAX_REG_POINTS) hipLaunchKernelGGL(lrg_fps_kernel<16>, g, blk, 0, s, n, m, inp, nullptr, out);
    else {
        if (!temp) return LRG_EINVAL - 3;
        hipLaunchKernelGGL(lrg_fps_kernel<0>, g, blk, 0, s, n, m, inp, temp, out);
    }
    LRG_LAUNCH_CHECK();
    return 0;
}

int lrg_gather_point(int b, int n, int m, const float *inp, const int *idx, float *out, void *stream) {
    if (b < 0 || n < 0 || m < 0) return LRG_EINVAL - 1;
    const long total = (long)b * m * 3;
    if (total == 0) return 0;
    if (!inp || !idx || !out) return LRG_EINVAL - 1;
    if (total < 0x7fffffffL - 256)
        hipLaunchKernelGGL(lrg_gather_point_kernel<int>, dim3(lrg_blocks(total, 256)), dim3(256), 0, (hipStream_t)stream, (int)total, n, m, inp, idx, out);
    else
        hipLaunchKernelGGL(lrg_gather_point_kernel<long>, dim3(lrg_blocks(total, 256)), dim3(256), 0, (hipStream_t)stream, total, n, m, inp, idx, out);
    LRG_LAUNCH_CHECK();
    return 0;
}

int lrg_scatter_add_point(int b, int n, int m, const float *out_g, const int *idx, float *inp_g, void *stream) {
    if (b < 0 || n < 0 || m < 0) return LRG_EINVAL - 1;
    const long total = (long)b * m * 3;
    if (total == 0) return 0;
    if (!out_g || !idx || !inp_g) return LRG_EINVAL - 1;
    if (total < 0x7fffffffL - 256)
        hipLaunchKernelGGL(lrg_scatter_add_point_kernel<int>, dim3(lrg_blocks(total, 256)), dim3(256), 0, (hipStream_t)stream, (int)total, n, m, out_g, idx, inp_g);
    else
        hipLaunchKernelGGL(lrg_scatter_add_point_kernel<long>, dim3(lrg_blocks(total, 256)), dim3(256), 0, (hipStream_t)stream, total, n, m, out_g, idx, inp_g);
    LRG_LAUNCH_CHECK();
    return 0;
}

int lrg_prob_sample(int b, int n, int m, const float *inp_p, const float *inp_r, float *temp, int *out, void *stream) {
    if (b < 0 || n < 0 || m < 0) return LRG_EINVAL - 1;
    if ((long)b * m == 0) return 0;
    if (n == 0 || !inp_p || !inp_r || !temp || !out) return LRG_EINVAL - 1;
    hipLaunchKernelGGL(lrg_cumsum_kernel, dim3((unsigned)b), dim3(1024), 0, (hipStream_t)stream, n, inp_p, temp);
    LRG_LAUNCH_CHECK();
    hipLaunchKernelGGL(lrg_binary_search_kernel, dim3(lrg_blocks((long)b * m, 256)), dim3(256), 0, (hipStream_t)stream, b, n, m, temp, inp_r, out);
    LRG_LAUNCH_CHECK();
    return 0;
}

int lrg_three_nn(int b, int n, int m, const float *xyz1, const float *xyz2, float *dist, int *idx, void *stream) {
    if (b < 0 || n < 0 || m < 0) return LRG_EINVAL - 1;
    if ((long)b * n == 0) return 0;
    if (!xyz1 || !dist || !idx || (m > 0 && !xyz2)) return LRG_EINVAL - 1;
    const int qb = (n + LRG_NN_THREADS - 1) / LRG_NN_THREADS;
    if ((long)b * qb > 0x7fffffffL) return LRG_EINVAL - 2;
    hipLaunchKernelGGL(lrg_three_nn_kernel, dim3((unsigned)(b * qb)), dim3(LRG_NN_THREADS), 0, (hipStream_t)stream, n, m, qb, xyz1, xyz2, dist, idx);
    LRG_LAUNCH_CHECK();
    return 0;
}

int lrg_three_interpolate(int b, int m, int c, int n, const float *points, const int *idx, const float *weight, float *out, void *stream) {
    if (b < 0 || m < 0 || c < 0 || n < 0) return LRG_EINVAL - 1;
    const long total = (long)b * n * c;
    if (total == 0) return 0;
    if (!idx || !weight || !out || (m > 0 && !points)) return LRG_EINVAL - 1;
    if (total < 0x7fffffffL - 256)
        hipLaunchKernelGGL(lrg_three_interpolate_kernel<int>, dim3(lrg_blocks(total, 256)), dim3(256), 0, (hipStream_t)stream, (int)total, m, c, n, points, idx, weight, out);
    else
        hipLaunchKernelGGL(lrg_three_interpolate_kernel<long>, dim3(lrg_blocks(total, 256)), dim3(256), 0, (hipStream_t)stream, total, m, c, n, points, idx, weight, out);
    LRG_LAUNCH_CHECK();
    return 0;
}

int lrg_three_interpolate_grad(int b, int n, int c, int m, const float *grad_out, const int *idx, const float *weight, float *grad_points, void *stream) {
    if (b < 0 || n < 0 || c < 0 || m < 0) return LRG_EINVAL - 1;
    const long total = (long)b * n * c;
    if (total == 0) return 0;
    if (!grad_out || !idx || !weight || (m > 0 && !grad_points)) return LRG_EINVAL - 1;
    if (total < 0x7fffffffL - 256)
        hipLaunchKernelGGL(lrg_three_interpolate_grad_kernel<int>, dim3(lrg_blocks(total, 256)), dim3(256), 0, (hipStream_t)stream, (int)total, n, c, m, grad_out, idx,
                           weight, grad_points);
    else
        hipLaunchKernelGGL(lrg_three_interpolate_grad_kernel<long>, dim3(lrg_blocks(total, 256)), dim3(256), 0, (hipStream_t)stream, total, n, c, m, grad_out, idx,
                           weight, grad_points);
    LRG_LAUNCH_CHECK();
    return 0;
}

int lrg_three_nn_interpolate(int b, int n, int m, int c, const float *xyz1, const float *xyz2, const float *points, float *dist, int *idx, float *weight,
                             float *out, void *stream) {
    if (b < 0 || n < 0 || m <= 0 || c < 0) return LRG_EINVAL - 1;
    if ((long)b * n == 0) return 0;
    if (!xyz1 || !xyz2 || (c > 0 && (!points || !out))) return LRG_EINVAL - 1;
    const int qb = (n + LRG_NN_THREADS - 1) / LRG_NN_THREADS;
    if ((long)b * qb > 0x7fffffffL || (long)LRG_NN_THREADS * c > 0x7fffffffL) return LRG_EINVAL - 2;
    hipLaunchKernelGGL(lrg_three_nn_interpolate_kernel, dim3((unsigned)(b * qb)), dim3(LRG_NN_THREADS), 0, (hipStream_t)stream, n, m, c, qb, xyz1, xyz2,
                       points, dist, idx, weight, out);
    LRG_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
