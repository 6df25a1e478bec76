// Training side of PointNet2 (train_pointnet.py:113-211) for gfx950: the one piece of its backward pass that the other entry points do
// not cover -- the gradients of group_point (tf_grouping_g.cu:61-78) and three_interpolate (tf_interpolate.cpp:131-155), which the
// reference accumulates with atomic additions, here in a FIXED order.  (The forward that keeps its layers is pn2_mlp_kernel's KEEP
// form in lrg_pointnet2.hip; everything else of the step is composed from lrg_train.hip and lrg_pointnet_train.hip.)
//
// out[b, idx[b, e], :] += weight[b, e] * grad[b, e / per, col0 : col0 + c], the sum over the entries e that name one source row taken in
// ASCENDING e.  A gather: nothing is added into memory, so nothing depends on scheduling.
//   invert   a workgroup owns one batch element and a slab of 256 source rows, thread t the row j = 256 * slab + t.  The element's
//            indices go to LDS once (an index outside [0, n) becomes row 0 or -1 = dropped, as the forward op it differentiates does).
//            Thread t walks them in ascending e and counts its own (every lane reads the same word: an LDS broadcast), an exclusive
//            scan over the 256 counts gives every row its place in the slab's list, a second walk writes the row's entries there --
//            in ascending e by construction, with no atomic of any kind.
//   sum      the slab's (row, column) pairs are dealt to the threads column-fastest (coalesced reads of grad's rows); each walks its
//            row's list in order: acc = acc + w[e] * g (a float32 multiplication, then a float32 addition, from 0), then
//            out = addend + acc (addend nullable), then out = 0 where mask <= 0 (nullable: the ReLU of the layer whose output this is
//            the gradient of).  A row nobody names gets 0, or the addend alone.
// LDS: 2 * entries * 4 bytes (dynamic), 64 KB for the largest level of the network (8192 entries), at most 128 KB.
#include "lrg_common.h"

#define SG_THREADS 256
#define SG_MAX_ENTRIES 16384
#define SG_LDS_MAX (2 * SG_MAX_ENTRIES * 4)

struct SgArgs {
    const float *grad, *weight, *addend, *mask;
    const int32_t *idx;
    float *out;
    int n, q, per, c, ldg, col0, drop, entries;
};

__global__ __launch_bounds__(SG_THREADS) void pn2_scatter_grad_kernel(SgArgs a) {
    extern __shared__ __attribute__((aligned(16))) int sg_lds[];          // src[entries], list[entries]
    __shared__ int s_scan[SG_THREADS], s_start[SG_THREADS], s_cnt[SG_THREADS];
    const int E = a.entries, t = threadIdx.x, b = blockIdx.y;
    const int j0 = blockIdx.x * SG_THREADS, j = j0 + t;
    int *src = sg_lds, *list = sg_lds + E;
    const int32_t *ib = a.idx + (long)b * E;
    for (int e = t; e < E; e += SG_THREADS) {
        int v = ib[e];
        if ((unsigned)v >= (unsigned)a.n) v = a.drop ? -1 : 0;
        src[e] = v;
    }
    __syncthreads();
    int cnt = 0;
    if (j < a.n)
        for (int e = 0; e < E; ++e) cnt += src[e] == j;
    s_scan[t] = cnt;
    __syncthreads();
    for (int d = 1; d < SG_THREADS; d <<= 1) {                            // inclusive scan of the 256 counts
        const int v = t >= d ? s_scan[t - d] : 0;
        __syncthreads();
        s_scan[t] += v;
        __syncthreads();
    }
    const int start = s_scan[t] - cnt;                                    // start + cnt <= the slab's total <= entries
    s_start[t] = start; s_cnt[t] = cnt;
    if (cnt > 0) {
        int k = start;
        const int end = start + cnt;
        for (int e = 0; e < E && k < end; ++e)
            if (src[e] == j) list[k++] = e;
    }
    __syncthreads();
    const int rows = min(SG_THREADS, a.n - j0), c = a.c;
    const float *gb = a.grad + (long)b * a.q * a.ldg + a.col0;
    const float *wb = a.weight ? a.weight + (long)b * E : nullptr;
    for (int item = t; item < rows * c; item += SG_THREADS) {
        const int jl = item / c, col = item - jl * c;
        const int *lp = list + s_start[jl];
        const int n_e = s_cnt[jl];
        float acc = 0.f;
        if (wb) {
            for (int k = 0; k < n_e; ++k) {
                const int e = lp[k];
                acc = __fadd_rn(acc, __fmul_rn(wb[e], gb[(long)(e / a.per) * a.ldg + col]));
            }
        } else {
            for (int k = 0; k < n_e; ++k) acc = __fadd_rn(acc, gb[(long)(lp[k] / a.per) * a.ldg + col]);
        }
        const long o = ((long)b * a.n + j0 + jl) * c + col;
        float v = a.addend ? __fadd_rn(a.addend[o], acc) : acc;
        if (a.mask && !(a.mask[o] > 0.f)) v = 0.f;
        a.out[o] = v;
    }
}

extern "C" {

int lrg_pointnet2_scatter_grad(int b, int n, int q, int per, int c, const float *grad, int ldg, int col0, const int32_t *idx,
                               const float *weight, int drop_out_of_range, const float *addend, const float *mask, float *out, void *stream) {
    if (b < 0 || b > 65535 || n < 1 || q < 1 || per < 1 || c < 1 || col0 < 0 || ldg < 1 || (long)col0 + c > ldg) return LRG_EINVAL - 2;
    if ((long)q * per > SG_MAX_ENTRIES || (long)SG_THREADS * c > 0x7fffffffL) return LRG_EINVAL - 2;
    if (drop_out_of_range != 0 && drop_out_of_range != 1) return LRG_EINVAL - 2;
    if (b == 0) return 0;
    if (!grad || !idx || !out) return LRG_EINVAL - 1;
    static bool attr_done[LRG_MAX_DEVICES] = {};
    const int dev = lrg_current_device();
    if (!attr_done[dev]) {
        LRG_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(pn2_scatter_grad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          SG_LDS_MAX));
        attr_done[dev] = true;
    }
    SgArgs a;
    a.grad = grad; a.weight = weight; a.addend = addend; a.mask = mask; a.idx = idx; a.out = out;
    a.n = n; a.q = q; a.per = per; a.c = c; a.ldg = ldg; a.col0 = col0; a.drop = drop_out_of_range; a.entries = q * per;
    const size_t lds = (size_t)2 * a.entries * sizeof(int);
    hipLaunchKernelGGL(pn2_scatter_grad_kernel, dim3((unsigned)((n + SG_THREADS - 1) / SG_THREADS), (unsigned)b), dim3(SG_THREADS), lds,
                       (hipStream_t)stream, a);
    LRG_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
