// Training side of the plain PointNet (train_pointnet.py:31-111) on gfx950: what its step needs beyond lrg_gemm_f32,
// lrg_pointwise_layer, lrg_segment_colsum and lrg_adam_step -- the batch norm of :63-93 in training mode (moments over the batch
// axis only, so one mean and one variance per (row position, channel)), its backward with the ReLU of :93 folded in, the sparse
// softmax cross entropy of :102-105 with its gradient, the head's input of :56-61 and its backward (the single-winner gradient of
// tf.nn.max_pool2d), and the moving averages of :71-78.  The step is sequenced by learn_region_grow_amd/pointnet_train.py.
//
// All of them are bandwidth-bound passes over [cells, 1024, c] tensors: a thread owns one (row position, channel) -- or one
// (cell, channel) -- and walks the other axis in ASCENDING order, consecutive threads own consecutive channels (a wavefront reads 64
// consecutive floats), and no sum goes through an atomic: the same inputs give the same bits.
#include "lrg_common.h"

#define PNT_CELL_ROWS 1024                   // POINTNET_NUM_POINT
#define PNT_MAX_BN_WIDTH 512                 // pointnet_variant's limit for a hidden fc width
#define PNT_MAX_CONV_WIDTH 1024
#define PNT_MAX_CLASSES 1024                 // lrg_pointnet_head's range
#define PNT_MAX_CELLS (1 << 20)
#define PNT_BN_EPSILON 1e-3f                 // :83

// ---- batch norm forward, is_training (:70, :83, :93) ----
// thread = (row position p, channel ch).  tf.nn.moments: mean over the cells, then the mean of (z - mean)^2 (biased, two passes).
// tf.nn.batch_normalization: inv = rsqrt(var + eps) * gamma; y = z * inv + (beta - mean * inv); then the ReLU of :93.
__global__ __launch_bounds__(256) void pnt_bn_forward_kernel(const float *z, const float *gamma, const float *beta, int cells, int c, float *y,
                                                             float *mean, float *var) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;          // p * c + ch
    const long plane = (long)PNT_CELL_ROWS * c;
    if (i >= plane) return;
    const int ch = (int)(i % c);
    float s = 0.f;
    for (int k = 0; k < cells; ++k) s += z[k * plane + i];
    const float mu = s / (float)cells;
    float q = 0.f;
    for (int k = 0; k < cells; ++k) {
        const float d = z[k * plane + i] - mu;
        q += d * d;
    }
    const float v = q / (float)cells;
    mean[i] = mu;
    var[i] = v;
    const float inv = (1.f / sqrtf(v + PNT_BN_EPSILON)) * gamma[ch];
    const float shift = beta[ch] - mu * inv;
    for (int k = 0; k < cells; ++k) y[k * plane + i] = fmaxf(z[k * plane + i] * inv + shift, 0.f);
}

// ---- batch norm backward, the ReLU folded in ----
// g = dy where y > 0; rstd = rsqrt(var + eps); xhat = (z - mean) rstd; per (p, ch): sg = sum_cells g, sgx = sum_cells g xhat,
// dz = gamma rstd (g - sg / cells - xhat sgx / cells).  sg and sgx go to the workspace ([2][1024][c]) for the second stage.
// dz may be dy itself (every element is read and then written by the thread that owns it).
__global__ __launch_bounds__(256) void pnt_bn_backward_kernel(const float *z, const float *y, const float *dy, const float *mean, const float *var,
                                                              const float *gamma, int cells, int c, float *dz, float *ws) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long plane = (long)PNT_CELL_ROWS * c;
    if (i >= plane) return;
    const int ch = (int)(i % c);
    const float mu = mean[i], rstd = 1.f / sqrtf(var[i] + PNT_BN_EPSILON);
    float sg = 0.f, sgx = 0.f;
    for (int k = 0; k < cells; ++k) {
        const long o = k * plane + i;
        const float g = y[o] > 0.f ? dy[o] : 0.f;
        const float xh = (z[o] - mu) * rstd;
        sg += g;
        sgx += g * xh;
    }
    ws[i] = sg;
    ws[plane + i] = sgx;
    const float mg = sg / (float)cells, mgx = sgx / (float)cells, scale = gamma[ch] * rstd;
    for (int k = 0; k < cells; ++k) {
        const long o = k * plane + i;
        const float g = y[o] > 0.f ? dy[o] : 0.f;
        const float xh = (z[o] - mu) * rstd;
        dz[o] = scale * ((g - mg) - xh * mgx) + 0.f;                     // + 0.f: a batch of one cell gives +0, never -0
    }
}

// Second stage: dbeta[ch] = sum_p sg[p][ch], dgamma[ch] = sum_p sgx[p][ch] in a fixed order: 64 channels x 4 row groups a workgroup,
// row group t sums p = 256 t .. 256 t + 255 ascending, then the four partial sums are added in the order 0, 1, 2, 3.
__global__ __launch_bounds__(256) void pnt_bn_reduce_kernel(const float *ws, int c, float *dbeta, float *dgamma) {
    __shared__ float part[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int ch = blockIdx.x * 64 + tx;
    const float *src = ws + (long)blockIdx.y * PNT_CELL_ROWS * c;
    float s = 0.f;
    if (ch < c)
        for (int p = ty * (PNT_CELL_ROWS / 4); p < (ty + 1) * (PNT_CELL_ROWS / 4); ++p) s += src[(long)p * c + ch];
    part[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && ch < c) {
        const float r = ((part[0][tx] + part[1][tx]) + part[2][tx]) + part[3][tx];
        (blockIdx.y == 0 ? dbeta : dgamma)[ch] = r;
    }
}

// ---- sparse softmax cross entropy (:102-105) ----
// One thread per row (13 classes: the 64 rows of a wavefront are 3.3 KB of consecutive memory).  A label outside [0, classes) gives a
// zero gradient row and is never used as an index.
__global__ __launch_bounds__(256) void pnt_softmax_grad_kernel(const float *logits, const int32_t *labels, long rows, int classes, float inv_rows,
                                                               float *dlogits) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const float *l = logits + r * classes;
    float *d = dlogits + r * classes;
    const int y = labels[r];
    if (y < 0 || y >= classes) {
        for (int k = 0; k < classes; ++k) d[k] = 0.f;
        return;
    }
    float m = l[0];
    for (int k = 1; k < classes; ++k) m = fmaxf(m, l[k]);
    float s = 0.f;
    for (int k = 0; k < classes; ++k) s += expf(l[k] - m);
    for (int k = 0; k < classes; ++k) d[k] = (expf(l[k] - m) / s - (k == y ? 1.f : 0.f)) * inv_rows;
}

// stats[0] += sum of the rows' losses, stats[1] += rows whose argmax (a tie to the lowest class, tf.argmax) is the label,
// stats[2] += rows whose label is outside [0, classes).  ONE workgroup: thread t takes rows t, t + 1024, ... in that order and the
// 1024 partial results meet in a fixed tree (lrg_ce_loss_kernel's scheme); thread 0 alone adds to stats, so nothing is atomic.
__global__ __launch_bounds__(1024) void pnt_softmax_loss_kernel(const float *logits, const int32_t *labels, long rows, int classes, double *stats) {
    __shared__ double sh[1024];
    __shared__ int shi[2][1024];
    double ce = 0.0;
    int ok = 0, bad = 0;
    for (long r = threadIdx.x; r < rows; r += 1024) {
        const float *l = logits + r * classes;
        const int y = labels[r];
        if (y < 0 || y >= classes) { ++bad; continue; }
        float m = l[0];
        int am = 0;
        for (int k = 1; k < classes; ++k)
            if (l[k] > m) { m = l[k]; am = k; }
        float s = 0.f;
        for (int k = 0; k < classes; ++k) s += expf(l[k] - m);
        ce += (double)(logf(s) + m - l[y]);
        ok += am == y;
    }
    sh[threadIdx.x] = ce; shi[0][threadIdx.x] = ok; shi[1][threadIdx.x] = bad;
    __syncthreads();
    for (int half = 512; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) {
            sh[threadIdx.x] += sh[threadIdx.x + half];
            shi[0][threadIdx.x] += shi[0][threadIdx.x + half];
            shi[1][threadIdx.x] += shi[1][threadIdx.x + half];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        stats[0] += sh[0];
        stats[1] += (double)shi[0][0];
        stats[2] += (double)shi[1][0];
    }
}

// ---- the head's first block (:56-59): t = conv_last - pooled[cell] ----
__global__ __launch_bounds__(256) void pnt_head_input_kernel(const float *last, const float *pooled, long total, int c, float *t) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;          // (cell * 1024 + p) * c + ch
    if (i >= total) return;
    const long cell = i / ((long)PNT_CELL_ROWS * c);
    t[i] = last[i] - pooled[cell * c + (int)(i % c)];
}

// ---- its backward: thread = (cell, ch) ----
// dlast = dt, and -S, S = the sum of dt over the cell's rows (ascending), on the FIRST row whose value equals pooled[cell, ch]: the
// single winner of a max-pool gradient.  addend (nullable, [cells,1024,c]) is a second gradient of the same tensor (the skip
// connection, when conv[1] is the last convolution); relu != 0 zeroes the result where last <= 0 (the last convolution's own ReLU,
// which its weight and bias gradients need applied).  dlast may be dt itself.
__global__ __launch_bounds__(256) void pnt_head_input_backward_kernel(const float *last, const float *pooled, const float *dt, const float *addend,
                                                                      int cells, int c, int relu, float *dlast) {
    const int ch = blockIdx.x * blockDim.x + threadIdx.x, cell = blockIdx.y;
    if (ch >= c) return;
    const long base = (long)cell * PNT_CELL_ROWS * c + ch;
    const float mx = pooled[(long)cell * c + ch];
    float s = 0.f;
    int win = -1;
    for (int p = 0; p < PNT_CELL_ROWS; ++p) {
        const long o = base + (long)p * c;
        s += dt[o];
        if (win < 0 && last[o] == mx) win = p;
    }
    for (int p = 0; p < PNT_CELL_ROWS; ++p) {
        const long o = base + (long)p * c;
        float v = dt[o];
        if (p == win) v -= s;
        if (addend) v += addend[o];
        if (relu && !(last[o] > 0.f)) v = 0.f;
        dlast[o] = v;
    }
}

// ---- ExponentialMovingAverage.apply (:71-78): shadow -= (shadow - value) * (1 - decay) ----
__global__ __launch_bounds__(256) void pnt_ema_kernel(float *shadow, const float *value, long n, float one_minus_decay) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    shadow[i] -= (shadow[i] - value[i]) * one_minus_decay;
}

static inline bool pnt_bn_shape_ok(int cells, int c) { return cells >= 1 && cells <= PNT_MAX_CELLS && c >= 32 && c <= PNT_MAX_BN_WIDTH && c % 32 == 0; }

extern "C" {

int lrg_pointnet_bn_forward(const float *z, const float *gamma, const float *beta, int cells, int c, float *y, float *mean, float *var,
                            void *stream) {
    if (!z || !gamma || !beta || !y || !mean || !var) return LRG_EINVAL - 1;
    if (!pnt_bn_shape_ok(cells, c)) return LRG_EINVAL - 2;
    const long plane = (long)PNT_CELL_ROWS * c;
    hipLaunchKernelGGL(pnt_bn_forward_kernel, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, (hipStream_t)stream, z, gamma, beta, cells, c, y,
                       mean, var);
    LRG_LAUNCH_CHECK();
    return 0;
}

size_t lrg_pointnet_bn_backward_workspace_bytes(int c) {
    if (c < 32 || c > PNT_MAX_BN_WIDTH || c % 32) return 0;
    return (size_t)2 * PNT_CELL_ROWS * c * sizeof(float);
}

int lrg_pointnet_bn_backward(const float *z, const float *y, const float *dy, const float *mean, const float *var, const float *gamma, int cells,
                             int c, float *dz, float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes, void *stream) {
    if (!z || !y || !dy || !mean || !var || !gamma || !dz || !dgamma || !dbeta || !workspace) return LRG_EINVAL - 1;
    if (!pnt_bn_shape_ok(cells, c)) return LRG_EINVAL - 2;
    if (workspace_bytes < lrg_pointnet_bn_backward_workspace_bytes(c)) return LRG_EINVAL - 3;
    const long plane = (long)PNT_CELL_ROWS * c;
    hipLaunchKernelGGL(pnt_bn_backward_kernel, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, (hipStream_t)stream, z, y, dy, mean, var, gamma,
                       cells, c, dz, (float *)workspace);
    LRG_LAUNCH_CHECK();
    hipLaunchKernelGGL(pnt_bn_reduce_kernel, dim3((c + 63) / 64, 2), dim3(256), 0, (hipStream_t)stream, (const float *)workspace, c, dbeta, dgamma);
    LRG_LAUNCH_CHECK();
    return 0;
}

int lrg_pointnet_softmax_ce_grad(const float *logits, const int32_t *labels, long rows, int classes, float *dlogits, double *stats, void *stream) {
    if (!logits || !labels || !stats) return LRG_EINVAL - 1;
    if (rows <= 0 || rows > ((long)1 << 31) - 1) return LRG_EINVAL - 2;
    if (classes < 1 || classes > PNT_MAX_CLASSES) return LRG_EINVAL - 3;
    if (dlogits) {                                                       // NULL: loss and counts only (evaluation)
        hipLaunchKernelGGL(pnt_softmax_grad_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, logits, labels, rows,
                           classes, 1.f / (float)rows, dlogits);
        LRG_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(pnt_softmax_loss_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, logits, labels, rows, classes, stats);
    LRG_LAUNCH_CHECK();
    return 0;
}

int lrg_pointnet_head_input(const float *last, const float *pooled, int cells, int c_last, float *t, void *stream) {
    if (!last || !pooled || !t) return LRG_EINVAL - 1;
    if (cells < 1 || cells > PNT_MAX_CELLS || c_last < 32 || c_last > PNT_MAX_CONV_WIDTH || c_last % 32) return LRG_EINVAL - 2;
    const long total = (long)cells * PNT_CELL_ROWS * c_last;
    if ((total + 255) / 256 > 0x7fffffffL) return LRG_EINVAL - 2;
    hipLaunchKernelGGL(pnt_head_input_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, last, pooled, total, c_last,
                       t);
    LRG_LAUNCH_CHECK();
    return 0;
}

int lrg_pointnet_head_input_backward(const float *last, const float *pooled, const float *dt, const float *addend, int cells, int c_last,
                                     int relu, float *dlast, void *stream) {
    if (!last || !pooled || !dt || !dlast) return LRG_EINVAL - 1;
    if (cells < 1 || cells > 65535 || c_last < 32 || c_last > PNT_MAX_CONV_WIDTH || c_last % 32) return LRG_EINVAL - 2;
    const int block = c_last < 256 ? c_last : 256;
    hipLaunchKernelGGL(pnt_head_input_backward_kernel, dim3((c_last + block - 1) / block, cells), dim3(block), 0, (hipStream_t)stream, last, pooled,
                       dt, addend, cells, c_last, relu, dlast);
    LRG_LAUNCH_CHECK();
    return 0;
}

int lrg_pointnet_ema_update(float *shadow, const float *value, long n, float one_minus_decay, void *stream) {
    if (!shadow || !value) return LRG_EINVAL - 1;
    if (n <= 0 || (n + 255) / 256 > 0x7fffffffL) return LRG_EINVAL - 2;
    hipLaunchKernelGGL(pnt_ema_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, shadow, value, n, one_minus_decay);
    LRG_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
