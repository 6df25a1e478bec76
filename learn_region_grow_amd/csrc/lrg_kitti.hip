// Fusing SemanticKITTI scans into scenes (stage_semantic_kitti.py of the reference), one sample per call, one thread per
// point in every launch.  All arithmetic is float64 and written as the plain chains DESIGN 3.19 states; the library is compiled with
// -ffp-contract=off, so no product and sum are fused, `/` is the IEEE division and rint rounds half to even.
//
//   lrg_kitti_project           world coordinates, the projection into the scan's image, the colour map and the two filters
//   lrg_kitti_first_in_voxel    the smallest index of every point's voxel (downsampling and equalisation)
//   lrg_kitti_components        26-neighbourhood components of the equalised points, joined from the unlabelled ones
//
// The tables are linear-probe hashes of lrg_pack_voxel keys with a power of two of at least 2 n slots, given by the caller.  A key
// is claimed by CAS and its value lowered by atomicMin, so a slot ends up with the smallest index that inserted its key, whatever
// the order of the threads; every probe loop ends after `slots` probes.  Unions are those of lrg_union.h (the root of a component is
// its minimum index); sizes are integer sums and first sources minima, so a call writes the same bytes every time.  Tables are read
// only by launches after the one that filled them.
#include "lrg_common.h"
#include "lrg_union.h"

#define KT_THREADS 256

struct KtProject {
    const float *scans; int ld; const int32_t *scan_of; const uint32_t *labels; int n, n_scans;
    const double *pose, *tr, *p2;
    const uint8_t *images; const int64_t *img_off; const int32_t *img_h, *img_w;
    double res;
    uint64_t *keys; int32_t *vals; int mask;
    double *xyz; uint8_t *rgb, *valid, *keep; int32_t *status;
};

__device__ __forceinline__ bool kt_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// rint(v / res) of the three coordinates as a packed key; LRG_HASH_EMPTY and a status bit when one is not finite or outside the window
__device__ __forceinline__ uint64_t kt_key(const double *p, double res, int32_t *status, int dx = 0, int dy = 0, int dz = 0) {
    int v[3];
    for (int c = 0; c < 3; ++c) {
        const double q = rint(p[c] / res);
        if (!kt_finite(q)) { atomicOr(status, LRG_KITTI_ST_NONFINITE); return LRG_HASH_EMPTY; }
        if (q < -(double)LRG_VOX_OFF + 1.0 || q > (double)LRG_VOX_OFF - 2.0) { atomicOr(status, LRG_KITTI_ST_WINDOW); return LRG_HASH_EMPTY; }
        v[c] = (int)q;
    }
    return lrg_pack_voxel(v[0] + dx, v[1] + dy, v[2] + dz);       // |v| <= 2^20 - 2: the 26 neighbours stay inside the window too
}

// key -> min(value, i); a full table sets a status bit (it cannot be full: slots >= 2 n)
__device__ __forceinline__ void kt_insert_min(uint64_t *keys, int32_t *vals, int mask, uint64_t key, int i, int32_t *status) {
    unsigned h = (unsigned)lrg_fmix64(key) & (unsigned)mask;
    for (int probe = 0; probe <= mask; ++probe) {
        unsigned long long prev = __hip_atomic_load(reinterpret_cast<unsigned long long *>(&keys[h]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (prev == LRG_HASH_EMPTY)
            prev = atomicCAS(reinterpret_cast<unsigned long long *>(&keys[h]), (unsigned long long)LRG_HASH_EMPTY, (unsigned long long)key);
        if (prev == LRG_HASH_EMPTY || prev == key) { atomicMin(&vals[h], i); return; }
        h = (h + 1) & (unsigned)mask;
    }
    atomicOr(status, LRG_KITTI_ST_TABLE);
}

__global__ __launch_bounds__(KT_THREADS) void kt_table_init_kernel(uint64_t *keys, int32_t *vals, long slots) {
    const long h = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= slots) return;
    keys[h] = LRG_HASH_EMPTY;
    vals[h] = INT_MAX;
}

// ((a0 x + a1 y) + a2 z) + a3 w
__device__ __forceinline__ double kt_chain(const double *a, double x, double y, double z, double w) {
    return ((a[0] * x + a[1] * y) + a[2] * z) + a[3] * w;
}

__global__ __launch_bounds__(KT_THREADS) void kt_project_kernel(KtProject a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const float *p = a.scans + (long)i * a.ld;
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    const int s = a.scan_of[i];
    if (s < 0 || s >= a.n_scans) {                   // checked on the host: this only keeps a bad word from turning into an address
        atomicOr(a.status, LRG_KITTI_ST_SCAN);
        a.valid[i] = 0;
        for (int c = 0; c < 3; ++c) { a.xyz[3L * i + c] = 0.0; a.rgb[3L * i + c] = 0; }
        return;
    }
    const double *m = a.pose + 12L * s;
    double w[3];
    for (int c = 0; c < 3; ++c) w[c] = ((m[4 * c] * x + m[4 * c + 1] * y) + m[4 * c + 2] * z) + m[4 * c + 3];
    for (int c = 0; c < 3; ++c) a.xyz[3L * i + c] = w[c];
    if (!kt_finite(w[0]) || !kt_finite(w[1]) || !kt_finite(w[2])) atomicOr(a.status, LRG_KITTI_ST_NONFINITE);
    // P2 (Tr [x y z 1]); the fourth row of Tr is 0 0 0 1
    double cam[4];
    for (int c = 0; c < 3; ++c) cam[c] = kt_chain(a.tr + 4 * c, x, y, z, 1.0);
    cam[3] = kt_chain(a.tr + 12, x, y, z, 1.0);
    double h[3];
    for (int c = 0; c < 3; ++c) h[c] = kt_chain(a.p2 + 4 * c, cam[0], cam[1], cam[2], cam[3]);
    const double u = rint(h[0] / h[2]), v = rint(h[1] / h[2]);
    const int W = a.img_w[s], H = a.img_h[s];
    const bool valid = h[2] > 0.0 && u >= 0.0 && u < (double)W && v >= 0.0 && v < (double)H;
    uint8_t c0 = 0, c1 = 0, c2 = 0;
    if (valid) {
        const uint8_t *px = a.images + a.img_off[s] + 3L * ((long)(int)v * W + (int)u);
        c0 = px[0]; c1 = px[1]; c2 = px[2];
    }
    a.rgb[3L * i] = c0; a.rgb[3L * i + 1] = c1; a.rgb[3L * i + 2] = c2;
    a.valid[i] = valid ? 1 : 0;
    if (valid) {
        const uint64_t key = kt_key(w, a.res, a.status);
        if (key != LRG_HASH_EMPTY) kt_insert_min(a.keys, a.vals, a.mask, key, i, a.status);
    }
}

// an invalid point takes the entry of its voxel when the entry's scan is not later than its own; then the two filters
__global__ __launch_bounds__(KT_THREADS) void kt_colour_kernel(KtProject a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    uint8_t c0 = a.rgb[3L * i], c1 = a.rgb[3L * i + 1], c2 = a.rgb[3L * i + 2];
    if (!a.valid[i]) {
        const uint64_t key = kt_key(a.xyz + 3L * i, a.res, a.status);
        const int j = lrg_hash_lookup(a.keys, a.vals, a.mask, key);
        // rgb[j] of a valid j was written by the launch before this one and is not written here
        if (j >= 0 && j < a.n && a.scan_of[j] <= a.scan_of[i]) {
            c0 = a.rgb[3L * j]; c1 = a.rgb[3L * j + 1]; c2 = a.rgb[3L * j + 2];
            a.rgb[3L * i] = c0; a.rgb[3L * i + 1] = c1; a.rgb[3L * i + 2] = c2;
        }
    }
    const uint32_t cls = a.labels[i] & 0xFFFFu;
    a.keep[i] = ((c0 | c1 | c2) != 0 && cls < 250u) ? 1 : 0;
}

static int kt_slots_ok(int n, int slots) { return slots >= 64 && (slots & (slots - 1)) == 0 && (long)slots >= 2L * n; }

extern "C" int lrg_kitti_table_slots(int n) {
    if (n < 0 || n > LRG_KITTI_MAX_POINTS) return 0;
    int slots = 64;
    while ((long)slots < 2L * n) slots <<= 1;
    return slots;
}

extern "C" int lrg_kitti_project(const float *scans, int ld, const int32_t *scan_of, const uint32_t *labels, int n, int n_scans, const double *pose,
                                 const double *tr, const double *p2, const uint8_t *images, const int64_t *img_off, const int32_t *img_h,
                                 const int32_t *img_w, double voxel_resolution, uint64_t *keys, int32_t *vals, int slots, double *xyz, uint8_t *rgb,
                                 uint8_t *valid, uint8_t *keep, int32_t *status, void *stream) {
    if (n < 0 || n > LRG_KITTI_MAX_POINTS || ld < 3 || n_scans < 1) return LRG_EINVAL - 110;
    if (!kt_slots_ok(n, slots) || !(voxel_resolution > 0.0)) return LRG_EINVAL - 111;
    if (!scans || !scan_of || !labels || !pose || !tr || !p2 || !images || !img_off || !img_h || !img_w || !keys || !vals || !xyz || !rgb || !valid ||
        !keep || !status)
        return LRG_EINVAL - 112;
    hipStream_t st = (hipStream_t)stream;
    LRG_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    KtProject a{scans, ld, scan_of, labels, n, n_scans, pose, tr, p2, images, img_off, img_h, img_w, voxel_resolution, keys, vals, slots - 1,
                xyz, rgb, valid, keep, status};
    hipLaunchKernelGGL(kt_table_init_kernel, dim3((slots + KT_THREADS - 1) / KT_THREADS), dim3(KT_THREADS), 0, st, keys, vals, (long)slots);
    if (n > 0) {
        const int g = (n + KT_THREADS - 1) / KT_THREADS;
        hipLaunchKernelGGL(kt_project_kernel, dim3(g), dim3(KT_THREADS), 0, st, a);
        hipLaunchKernelGGL(kt_colour_kernel, dim3(g), dim3(KT_THREADS), 0, st, a);
    }
    LRG_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct KtVoxel {
    const double *xyz; int n; double res;
    uint64_t *keys; int32_t *vals; int mask;
    int32_t *rep, *status;
};

__global__ __launch_bounds__(KT_THREADS) void kt_voxel_insert_kernel(KtVoxel a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const uint64_t key = kt_key(a.xyz + 3L * i, a.res, a.status);
    if (key != LRG_HASH_EMPTY) kt_insert_min(a.keys, a.vals, a.mask, key, i, a.status);
}

__global__ __launch_bounds__(KT_THREADS) void kt_voxel_rep_kernel(KtVoxel a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const uint64_t key = kt_key(a.xyz + 3L * i, a.res, a.status);
    const int j = lrg_hash_lookup(a.keys, a.vals, a.mask, key);
    a.rep[i] = (j >= 0 && j <= i) ? j : i;            // j < 0 only under a status bit
}

extern "C" int lrg_kitti_first_in_voxel(const double *xyz, int n, double resolution, uint64_t *keys, int32_t *vals, int slots, int32_t *rep,
                                        int32_t *status, void *stream) {
    if (n < 0 || n > LRG_KITTI_MAX_POINTS) return LRG_EINVAL - 113;
    if (!kt_slots_ok(n, slots) || !(resolution > 0.0)) return LRG_EINVAL - 114;
    if (!xyz || !keys || !vals || !rep || !status) return LRG_EINVAL - 115;
    hipStream_t st = (hipStream_t)stream;
    LRG_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    KtVoxel a{xyz, n, resolution, keys, vals, slots - 1, rep, status};
    hipLaunchKernelGGL(kt_table_init_kernel, dim3((slots + KT_THREADS - 1) / KT_THREADS), dim3(KT_THREADS), 0, st, keys, vals, (long)slots);
    if (n > 0) {
        const int g = (n + KT_THREADS - 1) / KT_THREADS;
        hipLaunchKernelGGL(kt_voxel_insert_kernel, dim3(g), dim3(KT_THREADS), 0, st, a);
        hipLaunchKernelGGL(kt_voxel_rep_kernel, dim3(g), dim3(KT_THREADS), 0, st, a);
    }
    LRG_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct KtComp {
    const double *xyz; const int32_t *obj, *cls; int n; double res;
    uint64_t *keys; int32_t *vals; int mask;
    int32_t *root, *size, *first_src; uint8_t *emits; int32_t *status;
};

__global__ __launch_bounds__(KT_THREADS) void kt_comp_init_kernel(KtComp a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    a.root[i] = i;
    a.size[i] = 0;
    a.first_src[i] = INT_MAX;
    a.emits[i] = 0;
}

// an unlabelled point joins every neighbour voxel's point of its class, labelled or not
__global__ __launch_bounds__(KT_THREADS) void kt_comp_union_kernel(KtComp a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n || a.obj[i] != 0) return;
    const int cls = a.cls[i];
    bool emits = false;
    for (int dx = -1; dx <= 1; ++dx)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dz = -1; dz <= 1; ++dz) {
                if (!dx && !dy && !dz) continue;
                const uint64_t key = kt_key(a.xyz + 3L * i, a.res, a.status, dx, dy, dz);
                const int k = lrg_hash_lookup(a.keys, a.vals, a.mask, key);
                if (k < 0 || k >= a.n || k == i || a.cls[k] != cls) continue;
                emits = true;
                bl_union(a.root, i, k);
            }
    if (emits) a.emits[i] = 1;
}

// every point's root (the parents are final after the union launch), the component's size and its smallest edge-emitting member
__global__ __launch_bounds__(KT_THREADS) void kt_comp_count_kernel(KtComp a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int root = bl_find(a.root, i);
    __hip_atomic_store(a.root + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    atomicAdd(&a.size[root], 1);
    if (a.emits[i]) atomicMin(&a.first_src[root], i);
}

extern "C" int lrg_kitti_components(const double *xyz, const int32_t *obj, const int32_t *cls, int n, double resolution, uint64_t *keys,
                                    int32_t *vals, int slots, int32_t *root, int32_t *size, int32_t *first_src, uint8_t *emits, int32_t *status,
                                    void *stream) {
    if (n < 0 || n > LRG_KITTI_MAX_POINTS) return LRG_EINVAL - 116;
    if (!kt_slots_ok(n, slots) || !(resolution > 0.0)) return LRG_EINVAL - 117;
    if (!xyz || !obj || !cls || !keys || !vals || !root || !size || !first_src || !emits || !status) return LRG_EINVAL - 118;
    hipStream_t st = (hipStream_t)stream;
    LRG_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    KtComp a{xyz, obj, cls, n, resolution, keys, vals, slots - 1, root, size, first_src, emits, status};
    KtVoxel v{xyz, n, resolution, keys, vals, slots - 1, nullptr, status};
    hipLaunchKernelGGL(kt_table_init_kernel, dim3((slots + KT_THREADS - 1) / KT_THREADS), dim3(KT_THREADS), 0, st, keys, vals, (long)slots);
    if (n > 0) {
        const int g = (n + KT_THREADS - 1) / KT_THREADS;
        hipLaunchKernelGGL(kt_comp_init_kernel, dim3(g), dim3(KT_THREADS), 0, st, a);
        hipLaunchKernelGGL(kt_voxel_insert_kernel, dim3(g), dim3(KT_THREADS), 0, st, v);
        hipLaunchKernelGGL(kt_comp_union_kernel, dim3(g), dim3(KT_THREADS), 0, st, a);
        hipLaunchKernelGGL(kt_comp_count_kernel, dim3(g), dim3(KT_THREADS), 0, st, a);
    }
    LRG_LAUNCH_CHECK();
    return 0;
}
