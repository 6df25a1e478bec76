// Training batches for LrgNet assembled on the device (train_region_grow.py:156-175; ABI 24): every tuple of a
// batch padded / subsampled to the network's k points per side, out of the flat row buffers that staging leaves on the device
// (lrg_stage_tuples) or that a staged file was uploaded into.  The draws are the counter stream's (lrg_rng.h), keyed by (rng_seed,
// tuple id) at (epoch, pass): a pure function of where they are used, so a batch does not depend on the batches before it.  Host
// twin: tests/assemble_ref.py.
#include "lrg_common.h"
#include "lrg_rng.h"

namespace {

#define LRG_ASSEMBLE_BT 256

// One workgroup per instance b: tuple t = order[b] with N = row_count[t] rows from row_start[t] on.  The k positions are computed
// once into LDS, then the k * F elements are copied with consecutive threads on consecutive output elements (a source row of 13 floats
// is 52 bytes: no 16-byte loads).  positives[b] = the sum of the k gathered labels, reduced over the workgroup: no atomics, the same
// bytes every time.
__global__ __launch_bounds__(LRG_ASSEMBLE_BT) void lrg_train_assemble_kernel(const float *rows, int row_stride, const int32_t *labels,
                                                                             const int64_t *row_start, const int32_t *row_count,
                                                                             const int32_t *order, int k, int F, uint32_t rng_seed,
                                                                             uint32_t epoch, uint32_t pass, uint32_t purpose, float *out_rows,
                                                                             int32_t *out_labels, int32_t *positives) {
    __shared__ uint32_t pos[LRG_ASSEMBLE_MAX_POINTS];
    __shared__ int part[LRG_ASSEMBLE_BT / 64];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int t = order[b];
    const uint32_t N = (uint32_t)row_count[t];
    const long base = row_start[t];
    int cnt = 0;
    for (int j = tid; j < k; j += LRG_ASSEMBLE_BT) {
        const uint32_t p = lrg_sample_position((uint32_t)j, N, (uint32_t)k, purpose, 0u, pass, epoch, rng_seed, (uint32_t)t);
        pos[j] = p;
        const int32_t lab = labels[base + p];
        out_labels[(long)b * k + j] = lab;
        cnt += lab;
    }
    cnt = lrg_wave_sum_i32(cnt);
    if (lrg_lane() == 0) part[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int w = 0; w < LRG_ASSEMBLE_BT / 64; ++w) s += part[w];
        positives[b] = s;
    }
    float *out = out_rows + (long)b * k * F;
    const int total = k * F;
    for (int x = tid; x < total; x += LRG_ASSEMBLE_BT) {
        const int j = x / F, c = x - j * F;
        out[x] = rows[(base + pos[j]) * row_stride + c];
    }
}

}  // namespace

extern "C" {

int lrg_train_assemble(const float *rows, int row_stride, const int32_t *labels, const int64_t *row_start, const int32_t *row_count,
                       const int32_t *order, int B, int k, int F, uint32_t rng_seed, int epoch, int pass, int purpose, float *out_rows,
                       int32_t *out_labels, int32_t *positives, void *stream) {
    if (!rows || !labels || !row_start || !row_count || !order || !out_rows || !out_labels || !positives) return LRG_EINVAL - 120;
    if (B < 1) return LRG_EINVAL - 121;
    if (k < 1 || k > LRG_ASSEMBLE_MAX_POINTS) return LRG_EINVAL - 122;
    if (F < 1 || F > (1 << 16)) return LRG_EINVAL - 123;
    if (F > row_stride) return LRG_EINVAL - 124;
    if (epoch < 0 || pass < 0 || pass > 0xFFFFFF || purpose < 0 || purpose > 0x7F) return LRG_EINVAL - 125;
    hipLaunchKernelGGL(lrg_train_assemble_kernel, dim3(B), dim3(LRG_ASSEMBLE_BT), 0, (hipStream_t)stream, rows, row_stride, labels, row_start,
                       row_count, order, k, F, rng_seed, (uint32_t)epoch, (uint32_t)pass, (uint32_t)purpose, out_rows, out_labels, positives);
    LRG_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
