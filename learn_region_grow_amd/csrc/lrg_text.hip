// The vertex lines of savePLY / savePCD encoded on the device (include/lrg_hip.h: lrg_text_encode; the arithmetic of a
// field is csrc/lrg_text_fmt.h).  Three steps on the caller's stream: a LENGTH pass (one line length per row, 0 for a refused row, the
// refused rows counted), the project's exclusive scan over the lengths (lrg_scan.hip), and a WRITE pass.
//
// Write pass: one row per lane, TEXT_THREADS rows per workgroup.  The rows of a workgroup are consecutive, so its lines are one
// contiguous run [lo, hi) of the output.  Every lane builds its line in an LDS tile at the place it has in that run, the tile laid over
// the output from the 16-byte boundary at or below lo, so that byte g of the output is tile[g - (lo & ~15)]; behind one barrier the
// workgroup copies the run out 16 bytes per lane and store, each store aligned in LDS and in memory alike.  The first and the last
// 16-byte piece of a run belong in part to the neighbouring workgroups: those two go out byte by byte, only the bytes in [lo, hi).
#include "lrg_common.h"
#include "lrg_text_fmt.h"

#define TEXT_THREADS 256
#define TEXT_RUN_MAX (TEXT_THREADS * LRG_TEXT_MAX_LINE)
#define TEXT_TILE (TEXT_RUN_MAX + 16)

__device__ __forceinline__ void text_load_row(const float *xyz, int ld, const int32_t *rgb, int i, int format, LrgTextRow *r) {
    const float *p = xyz + (size_t)i * ld;
    const uint32_t bits[3] = {__float_as_uint(p[0]), __float_as_uint(p[1]), __float_as_uint(p[2])};
    const int32_t col[3] = {rgb[3 * (size_t)i], rgb[3 * (size_t)i + 1], rgb[3 * (size_t)i + 2]};
    lrg_text_row(bits, col, format, r);
}

// len [n + 1]: the line length of every row and a closing 0, so that the scan of n + 1 entries ends in the total
__global__ __launch_bounds__(TEXT_THREADS) void text_len_kernel(const float *xyz, int ld, const int32_t *rgb, int n, int format, int32_t *len,
                                                                 int32_t *status) {
    const int i = blockIdx.x * TEXT_THREADS + threadIdx.x;
    int refused = 0;
    if (i < n) {
        LrgTextRow r;
        text_load_row(xyz, ld, rgb, i, format, &r);
        len[i] = r.len;
        refused = r.len == 0;
    } else if (i == n) len[n] = 0;
    const int cnt = __syncthreads_count(refused);
    if (threadIdx.x == 0 && cnt) atomicAdd(status, cnt);
}

__global__ __launch_bounds__(TEXT_THREADS) void text_write_kernel(const float *xyz, int ld, const int32_t *rgb, int n, int format,
                                                                   const int32_t *line_off, uint8_t *text, size_t text_bytes) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[TEXT_TILE];
    const int first = blockIdx.x * TEXT_THREADS, last = min(n, first + TEXT_THREADS);
    const int lo = line_off[first], hi = line_off[last];
    if (lo < 0 || hi < lo || hi - lo > TEXT_RUN_MAX || (size_t)hi > text_bytes) return;      // (uniform; cannot happen: no line is longer than LRG_TEXT_MAX_LINE)
    const int base = lo & ~15;
    const int i = first + threadIdx.x;
    if (i < last) {
        LrgTextRow r;
        text_load_row(xyz, ld, rgb, i, format, &r);
        const int at = line_off[i] - base;
        if (r.len && at >= 0 && at + r.len <= TEXT_TILE) lrg_text_put_row(tile + at, r);
    }
    __syncthreads();
    for (int g = base + 16 * (int)threadIdx.x; g < hi; g += 16 * TEXT_THREADS) {
        if (g >= lo && g + 16 <= hi) *(uint4 *)(text + g) = *(const uint4 *)(tile + (g - base));
        else
            for (int b = max(g, lo); b < min(g + 16, hi); ++b) text[b] = tile[b - base];
    }
}

static void text_layout(int n, size_t *len, size_t *bsum, size_t *total) {
    LrgArena ws;
    *len = ws.take(((size_t)n + 1) * 4);
    *bsum = ws.take((size_t)(lrg_scan_blocks((long)n + 1) + 1) * 4);
    *total = ws.total;
}

extern "C" size_t lrg_text_workspace_bytes(int n) {
    size_t len, bsum, total;
    text_layout(n < 0 ? 0 : n, &len, &bsum, &total);
    return total;
}

extern "C" int lrg_text_encode(const float *xyz, int ld, const int32_t *rgb, int n, int format, void *workspace, size_t workspace_bytes,
                               int32_t *line_off, uint8_t *text, size_t text_bytes, int32_t *status, void *stream) {
    if (!line_off || !status || !workspace || ((uintptr_t)workspace & 15)) return LRG_EINVAL - 130;
    if (n < 0 || (long)n * LRG_TEXT_MAX_LINE >= (1l << 31)) return LRG_EINVAL - 131;
    if (n > 0 && (!xyz || !rgb || !text || ((uintptr_t)text & 15))) return LRG_EINVAL - 130;
    if (ld < 3) return LRG_EINVAL - 132;
    if (format != LRG_TEXT_PLY && format != LRG_TEXT_PCD) return LRG_EINVAL - 133;
    size_t o_len, o_bsum, total;
    text_layout(n, &o_len, &o_bsum, &total);
    if (workspace_bytes < total || text_bytes < (size_t)n * LRG_TEXT_MAX_LINE) return LRG_EINVAL - 134;
    hipStream_t st = (hipStream_t)stream;
    LRG_HIP_CHECK(hipMemsetAsync(status, 0, 4, st));
    if (n == 0) {
        LRG_HIP_CHECK(hipMemsetAsync(line_off, 0, 4, st));
        return 0;
    }
    int32_t *len = (int32_t *)((char *)workspace + o_len), *bsum = (int32_t *)((char *)workspace + o_bsum);
    hipLaunchKernelGGL(text_len_kernel, dim3(n / TEXT_THREADS + 1), dim3(TEXT_THREADS), 0, st, xyz, ld, rgb, n, format, len, status);
    LRG_LAUNCH_CHECK();
    int rc;
    if ((rc = lrg_exscan_i32(len, (long)n + 1, bsum, line_off, st))) return rc;
    hipLaunchKernelGGL(text_write_kernel, dim3((n + TEXT_THREADS - 1) / TEXT_THREADS), dim3(TEXT_THREADS), 0, st, xyz, ld, rgb, n, format,
                       (const int32_t *)line_off, text, text_bytes);
    LRG_LAUNCH_CHECK();
    return 0;
}
