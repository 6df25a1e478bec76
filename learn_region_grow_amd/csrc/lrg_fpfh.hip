// Fast Point Feature Histograms of benchmarks.py --mode fpfh (:354-358), without PCL, for gfx950.  DESIGN.md §3.15 is the
// definition: PCL's FPFHEstimation arithmetic in float32 on the +-2 voxel window of an equalised room.
//
// A batch of rooms goes through a fixed sequence of launches, one point per lane in each:
//   init     hash slots empty, status cleared, the room of every point (binary search in room_start)
//   insert   voxel key -> the room's own linear-probe segment (lrg_room_hash.h); a key met twice is an error
//   pairs    125 window lookups; every j with d2 <= r2 counts in k; every pair j != i goes through computePairFeatures and
//            increments three of the lane's 33 counters.  The counters live in LDS, one row of 33 words per lane: lane l's word b
//            is on bank (l + b) % 32, so the 32 lanes of a half-wave never meet on a bank whatever their b, and a row has one
//            owner, so no atomics.  (33 counters in registers would be indexed dynamically, i.e. spilled.)
//   gather   the window again (or the neighbour list the pairs pass stored, LRG_FPFH_LISTS): acc[b] += spfh_j[b] / d2 in
//            window order and float64, then each block of 11 bins scaled to sum 100 and rounded to float32.  The neighbours'
//            counters are read as bytes (k <= 125, so a counter is at most 124): 9 words a neighbour instead of 33.
// Nothing is accumulated by float atomics and the order of every sum is the window's, so the output is a function of the room
// alone: not of the batch, the launch or the run.
#include "lrg_common.h"
#include "lrg_room_hash.h"

#define FP_THREADS 256
#define FP_BINS 33
#define FP_BYTES 36                           // a point's byte counters, padded to 9 words
#define FP_LIST_CAP 48                        // neighbours stored per point with LRG_FPFH_LISTS; a longer list is probed again
enum { FP_ST_WINDOW = 1, FP_ST_DUPLICATE = 2 };          // the meanings of lrg_baseline_status

struct LrgFpfhLayout {
    size_t keys, vals, rooms, room_of, bytes, lists, scal, total;
    long hslots;
};

static int fp_layout(int N, int R, int flags, LrgFpfhLayout *L) {
    if (N < 0 || R < 0 || N > (1 << 26) || R > (1 << 20)) return LRG_EINVAL - 90;
    if (flags & ~LRG_FPFH_LISTS) return LRG_EINVAL - 90;
    L->hslots = lrg_room_hash_slots(N, R);
    LrgArena ws;
    L->keys = ws.take((size_t)L->hslots * 8);
    L->vals = ws.take((size_t)L->hslots * 4);
    L->rooms = ws.take((size_t)(R + 1) * 4);
    L->room_of = ws.take((size_t)N * 4);
    L->bytes = ws.take((size_t)N * FP_BYTES);
    L->lists = ws.take((flags & LRG_FPFH_LISTS) ? (size_t)N * FP_LIST_CAP * 4 : 0);
    L->scal = ws.take(64 * 4);
    L->total = ws.total;
    return 0;
}

struct FpArgs {
    const float *pts; int ld;
    const float *xyz, *nrm;
    const int32_t *room_start; int n_rooms, n;
    float res, r2;
    uint64_t *keys; int32_t *vals, *room_of; uint32_t *bytes; int32_t *lists, *scal;
    long hslots;
    int32_t *counts, *k; float *fpfh;
};

__global__ __launch_bounds__(FP_THREADS) void fp_init_kernel(FpArgs a) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < a.hslots) { a.keys[t] = LRG_HASH_EMPTY; a.vals[t] = -1; }
    if (t < 64) a.scal[t] = 0;
    if (t < a.n) a.room_of[t] = lrg_room_of(a.room_start, a.n_rooms, (int)t);
}

__global__ __launch_bounds__(FP_THREADS) void fp_insert_kernel(FpArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int r = a.room_of[i];
    int s, e;
    if (!lrg_room_bounds(a.room_start, a.n, r, &s, &e)) { a.room_of[i] = -1; return; }
    const float *p = a.pts + (long)i * a.ld;
    const uint64_t key = lrg_pack_voxel(lrg_voxel_of(p[0], a.res), lrg_voxel_of(p[1], a.res), lrg_voxel_of(p[2], a.res));
    if (key == LRG_HASH_EMPTY) { atomicOr(&a.scal[0], FP_ST_WINDOW); a.room_of[i] = -1; return; }
    uint64_t *keys; int32_t *vals; int mask;
    lrg_room_segment(a.keys, a.vals, r, s, e, &keys, &vals, &mask);
    if (!lrg_room_insert(keys, vals, mask, key, i)) atomicOr(&a.scal[0], FP_ST_DUPLICATE);      // the room is not equalised
}

// floor(11 x) clamped to [0, 10]; a NaN goes to bin 0 (fmaxf returns its other argument), so the result is always a valid index
__device__ __forceinline__ int fp_bin(float x) { return (int)fminf(fmaxf(floorf(__fmul_rn(11.f, x)), 0.f), 10.f); }

// d2 = (dx dx + dy dy) + dz dz in float32, d = P[j] - P[i]
__device__ __forceinline__ float fp_dist2(const float *xyz, int i, int j, float *dx, float *dy, float *dz) {
    const float *p = xyz + 3L * i, *q = xyz + 3L * j;
    *dx = __fsub_rn(q[0], p[0]); *dy = __fsub_rn(q[1], p[1]); *dz = __fsub_rn(q[2], p[2]);
    return __fadd_rn(__fadd_rn(__fmul_rn(*dx, *dx), __fmul_rn(*dy, *dy)), __fmul_rn(*dz, *dz));
}

__device__ __forceinline__ float fp_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return __fadd_rn(__fadd_rn(__fmul_rn(ax, bx), __fmul_rn(ay, by)), __fmul_rn(az, bz));
}

// PCL's computePairFeatures for p1 = P[i], p2 = P[j]; false when the pair is skipped
__device__ __forceinline__ bool fp_pair_bins(const float *nrm, int i, int j, float dx, float dy, float dz, float d2, int *b1, int *b2, int *b3) {
    const float f4 = __fsqrt_rn(d2);
    if (f4 == 0.f) return false;
    float n1x = nrm[3L * i], n1y = nrm[3L * i + 1], n1z = nrm[3L * i + 2];
    float n2x = nrm[3L * j], n2y = nrm[3L * j + 1], n2z = nrm[3L * j + 2];
    const float a1 = __fdiv_rn(fp_dot(n1x, n1y, n1z, dx, dy, dz), f4), a2 = __fdiv_rn(fp_dot(n2x, n2y, n2z, dx, dy, dz), f4);
    float f3 = a1;
    if (fabsf(a1) < fabsf(a2)) {                    // acos(|a1|) > acos(|a2|): the frame goes to the other point
        float t;
        t = n1x; n1x = n2x; n2x = t;
        t = n1y; n1y = n2y; n2y = t;
        t = n1z; n1z = n2z; n2z = t;
        dx = -dx; dy = -dy; dz = -dz;
        f3 = -a2;
    }
    float vx = __fsub_rn(__fmul_rn(dy, n1z), __fmul_rn(dz, n1y));           // v = d x n1
    float vy = __fsub_rn(__fmul_rn(dz, n1x), __fmul_rn(dx, n1z));
    float vz = __fsub_rn(__fmul_rn(dx, n1y), __fmul_rn(dy, n1x));
    const float vn = __fsqrt_rn(fp_dot(vx, vy, vz, vx, vy, vz));
    if (vn == 0.f) return false;
    vx = __fdiv_rn(vx, vn); vy = __fdiv_rn(vy, vn); vz = __fdiv_rn(vz, vn);
    const float wx = __fsub_rn(__fmul_rn(n1y, vz), __fmul_rn(n1z, vy));     // w = n1 x v
    const float wy = __fsub_rn(__fmul_rn(n1z, vx), __fmul_rn(n1x, vz));
    const float wz = __fsub_rn(__fmul_rn(n1x, vy), __fmul_rn(n1y, vx));
    const float f2 = fp_dot(vx, vy, vz, n2x, n2y, n2z);
    const float f1 = atan2f(fp_dot(wx, wy, wz, n2x, n2y, n2z), fp_dot(n1x, n1y, n1z, n2x, n2y, n2z));
    const float pi = 3.14159265358979323846f;
    *b1 = fp_bin(__fdiv_rn(__fadd_rn(f1, pi), __fmul_rn(2.f, pi)));
    *b2 = fp_bin(__fdiv_rn(__fadd_rn(f2, 1.f), 2.f));
    *b3 = fp_bin(__fdiv_rn(__fadd_rn(f3, 1.f), 2.f));
    return true;
}

__global__ __launch_bounds__(FP_THREADS) void fp_pairs_kernel(FpArgs a) {
    __shared__ int32_t cnt[FP_THREADS * FP_BINS];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    int32_t *row = cnt + threadIdx.x * FP_BINS;
    for (int b = 0; b < FP_BINS; ++b) row[b] = 0;                          // the lane's own row: no barrier anywhere
    if (i >= a.n) return;
    int k = 0, m = 0;
    const int r = a.room_of[i];
    int s, e;
    if (r >= 0 && lrg_room_bounds(a.room_start, a.n, r, &s, &e)) {
        uint64_t *keys; int32_t *vals; int mask;
        lrg_room_segment(a.keys, a.vals, r, s, e, &keys, &vals, &mask);
        const float *p = a.pts + (long)i * a.ld;
        const int vx = lrg_voxel_of(p[0], a.res), vy = lrg_voxel_of(p[1], a.res), vz = lrg_voxel_of(p[2], a.res);
        for (int ox = -2; ox <= 2; ++ox)
            for (int oy = -2; oy <= 2; ++oy)
                for (int oz = -2; oz <= 2; ++oz) {
                    const int j = (ox | oy | oz) ? lrg_hash_lookup(keys, vals, mask, lrg_pack_voxel(vx + ox, vy + oy, vz + oz)) : i;
                    if (j < s || j >= e) continue;                        // empty, or (never, by the segment) another room's
                    float dx, dy, dz;
                    const float d2 = fp_dist2(a.xyz, i, j, &dx, &dy, &dz);
                    if (!(d2 <= a.r2)) continue;
                    ++k;
                    if (j == i) continue;
                    if (a.lists && m < FP_LIST_CAP) a.lists[(long)i * FP_LIST_CAP + m] = j;
                    ++m;
                    int b1, b2, b3;
                    if (!fp_pair_bins(a.nrm, i, j, dx, dy, dz, d2, &b1, &b2, &b3)) continue;
                    ++row[b1]; ++row[11 + b2]; ++row[22 + b3];
                }
    }
    a.k[i] = k;
    uint32_t word = 0;
    for (int b = 0; b < FP_BYTES; ++b) {
        const int c = b < FP_BINS ? row[b] : 0;
        if (b < FP_BINS) a.counts[(long)i * FP_BINS + b] = c;
        word |= (uint32_t)c << (8 * (b & 3));
        if ((b & 3) == 3) { a.bytes[(long)i * (FP_BYTES / 4) + (b >> 2)] = word; word = 0; }
    }
}

// acc[b] += spfh_j[b] * (1 / d2), spfh_j[b] = float(c_j[b]) * (100 / (k_j - 1)) in float32, the rest in float64: j != i and d2 <= r2
// give k_j >= 2.  The float64 sums make a block with one occupied bin come out at exactly 100 (x * (100 / x) is 100 to within 2^-52).
__device__ __forceinline__ void fp_add(const FpArgs &a, int j, float d2, double *acc) {
    const float scale = __fdiv_rn(100.f, (float)(a.k[j] - 1));
    const double wgt = __ddiv_rn(1.0, (double)d2);
    const uint32_t *src = a.bytes + (long)j * (FP_BYTES / 4);
#pragma unroll
    for (int q = 0; q < FP_BYTES / 4; ++q) {
        const uint32_t word = src[q];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int b = 4 * q + c;
            if (b < FP_BINS)
                acc[b] = __dadd_rn(acc[b], __dmul_rn((double)__fmul_rn((float)((word >> (8 * c)) & 0xffu), scale), wgt));
        }
    }
}

__global__ __launch_bounds__(FP_THREADS) void fp_gather_kernel(FpArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    double acc[FP_BINS];
#pragma unroll
    for (int b = 0; b < FP_BINS; ++b) acc[b] = 0.0;
    const int r = a.room_of[i];
    int s, e;
    if (r >= 0 && lrg_room_bounds(a.room_start, a.n, r, &s, &e)) {
        const int m = a.k[i] - 1;                                          // the pairs pass counted i itself
        if (a.lists && m <= FP_LIST_CAP) {
            for (int q = 0; q < m; ++q) {
                const int j = a.lists[(long)i * FP_LIST_CAP + q];
                if (j < s || j >= e) continue;
                float dx, dy, dz;
                fp_add(a, j, fp_dist2(a.xyz, i, j, &dx, &dy, &dz), acc);
            }
        } else if (m > 0) {
            uint64_t *keys; int32_t *vals; int mask;
            lrg_room_segment(a.keys, a.vals, r, s, e, &keys, &vals, &mask);
            const float *p = a.pts + (long)i * a.ld;
            const int vx = lrg_voxel_of(p[0], a.res), vy = lrg_voxel_of(p[1], a.res), vz = lrg_voxel_of(p[2], a.res);
            for (int ox = -2; ox <= 2; ++ox)
                for (int oy = -2; oy <= 2; ++oy)
                    for (int oz = -2; oz <= 2; ++oz) {
                        if (!(ox | oy | oz)) continue;
                        const int j = lrg_hash_lookup(keys, vals, mask, lrg_pack_voxel(vx + ox, vy + oy, vz + oz));
                        if (j < s || j >= e || j == i) continue;
                        float dx, dy, dz;
                        const float d2 = fp_dist2(a.xyz, i, j, &dx, &dy, &dz);
                        if (!(d2 <= a.r2)) continue;
                        fp_add(a, j, d2, acc);
                    }
        }
    }
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        double sum = 0.0;
#pragma unroll
        for (int b = 0; b < 11; ++b) sum = __dadd_rn(sum, acc[11 * g + b]);
        const double f = sum != 0.0 ? __ddiv_rn(100.0, sum) : 1.0;
#pragma unroll
        for (int b = 0; b < 11; ++b) a.fpfh[(long)i * FP_BINS + 11 * g + b] = (float)(sum != 0.0 ? __dmul_rn(acc[11 * g + b], f) : acc[11 * g + b]);
    }
}

extern "C" {

size_t lrg_fpfh_workspace_bytes(int n_points, int n_rooms, int flags) {
    LrgFpfhLayout L;
    if (fp_layout(n_points, n_rooms, flags, &L)) return 0;
    return L.total;
}

int lrg_fpfh(const float *pts, int ld, const float *xyz, const float *normals, const int32_t *room_start, int n_rooms, float resolution,
             float radius, int flags, void *ws, size_t ws_bytes, int32_t *counts, int32_t *k, float *fpfh, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n_rooms < 1 || n_rooms > (1 << 20) || !room_start || room_start[0] != 0) return LRG_EINVAL - 91;
    for (int r = 0; r < n_rooms; ++r)
        if (room_start[r + 1] < room_start[r]) return LRG_EINVAL - 91;
    const int n = room_start[n_rooms];
    LrgFpfhLayout L;
    int rc = fp_layout(n, n_rooms, flags, &L);
    if (rc) return rc;
    if (!(resolution > 0.f) || !(radius > 0.f)) return LRG_EINVAL - 92;
    if (radius > 2.f * resolution) return LRG_EINVAL;                    // the +-2 voxel window could not hold such a ball
    if (!ws || ws_bytes < L.total || ((uintptr_t)ws & 255)) return LRG_EINVAL - 93;
    if (n > 0 && (!pts || ld < 3 || !xyz || !normals || !counts || !k || !fpfh)) return LRG_EINVAL - 91;
    char *w = static_cast<char *>(ws);
    FpArgs a;
    int32_t *rooms = reinterpret_cast<int32_t *>(w + L.rooms);           // a device copy of room_start (the caller's is host memory)
    LRG_HIP_CHECK(hipMemcpyAsync(rooms, room_start, (size_t)(n_rooms + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
    a.pts = pts; a.ld = ld; a.xyz = xyz; a.nrm = normals; a.room_start = rooms; a.n_rooms = n_rooms; a.n = n;
    a.res = resolution; a.r2 = radius * radius;
    a.keys = reinterpret_cast<uint64_t *>(w + L.keys); a.vals = reinterpret_cast<int32_t *>(w + L.vals);
    a.room_of = reinterpret_cast<int32_t *>(w + L.room_of); a.bytes = reinterpret_cast<uint32_t *>(w + L.bytes);
    a.lists = (flags & LRG_FPFH_LISTS) ? reinterpret_cast<int32_t *>(w + L.lists) : nullptr;
    a.scal = reinterpret_cast<int32_t *>(w + L.scal); a.hslots = L.hslots;
    a.counts = counts; a.k = k; a.fpfh = fpfh;
    const long init_n = L.hslots > (long)n + 64 ? L.hslots : (long)n + 64;
    hipLaunchKernelGGL(fp_init_kernel, dim3((unsigned)((init_n + FP_THREADS - 1) / FP_THREADS)), dim3(FP_THREADS), 0, st, a);
    if (n > 0) {
        const int gn = (n + FP_THREADS - 1) / FP_THREADS;
        hipLaunchKernelGGL(fp_insert_kernel, dim3(gn), dim3(FP_THREADS), 0, st, a);
        hipLaunchKernelGGL(fp_pairs_kernel, dim3(gn), dim3(FP_THREADS), 0, st, a);
        hipLaunchKernelGGL(fp_gather_kernel, dim3(gn), dim3(FP_THREADS), 0, st, a);
    }
    LRG_LAUNCH_CHECK();
    return 0;
}

int lrg_fpfh_status(const void *ws, int n_points, int n_rooms, int flags, int32_t *host_status, void *stream) {
    LrgFpfhLayout L;
    int rc = fp_layout(n_points, n_rooms, flags, &L);
    if (rc) return rc;
    if (!ws || !host_status) return LRG_EINVAL - 91;
    LRG_HIP_CHECK(hipMemcpyAsync(host_status, static_cast<const char *>(ws) + L.scal, sizeof(int32_t), hipMemcpyDeviceToHost,
                                 (hipStream_t)stream));
    LRG_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

}  // extern "C"
