// Room preprocessing P0 on the GPU (test_region_grow.py:119-173): first-point-per-voxel equalisation, per-point PCA over
// the raw points of the 27 surrounding voxels, the 13-column feature stack.
//
// Everything up to and including the covariance matrix is computed in the reference's own arithmetic AND order -- voxel
// of a point = rint(float32 x / float32 res); neighbours visited in itertools.product([-1,0,1]^3) order, raw points in
// file order inside a voxel; float32 outer products accumulated in float64; cov = accA/n - outer(accB,accB)/n^2 -- so the
// covariances are bit-identical to the NumPy loop.  The 3x3 decomposition is where a GPU cannot follow the reference
// (LAPACK dgesdd inside numpy.linalg.svd): eig_mode 0 stops after the covariances (the host runs the same LAPACK call:
// bit-exact features), eig_mode 1 solves them here with a cyclic Jacobi iteration in float64 (|error| ~ 1e-16 |cov|:
// features agree to float32 rounding, documented tolerance in tests/test_gpu_preprocess.py).
//
// ONE pipeline: all rooms of a file in one pass (lrg_preprocess_batch); lrg_preprocess and its companions are that pass
// with one room.
#include "lrg_common.h"
#include "lrg_eig3.h"
#include "lrg_room_hash.h"

#define PREP_THREADS 256

// ---- order-preserving integer images of floats / doubles (for atomicMin / atomicMax) ----
__device__ __forceinline__ int prep_ord(float f) { int i = __float_as_int(f); return i >= 0 ? i : i ^ 0x7fffffff; }
__device__ __forceinline__ float prep_unord(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }

__global__ void prep_flag_kernel(const int32_t *slot_of, const int32_t *first, int M, int32_t *flag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < M) flag[i] = (slot_of[i] >= 0 && first[slot_of[i]] == i) ? 1 : 0;
}

// raw points of a voxel in file order (normal_grid[k].append(i), :131-133)
__global__ void prep_sort_lists_kernel(const int32_t *hash_off, const int32_t *count, int cap, int32_t *list) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= cap) return;
    const int n = count[s];
    if (n < 2) return;
    int32_t *a = list + hash_off[s];
    for (int i = 1; i < n; ++i) {
        const int v = a[i];
        int j = i - 1;
        while (j >= 0 && a[j] > v) { a[j + 1] = a[j]; --j; }
        a[j + 1] = v;
    }
}

// The arithmetic of one equalised point: covariance of the raw points in the 27 voxels around pe (:144-157).  keys / hash_off /
// count are the room's hash segment; list and raw are indexed as hash_off says (file-wide).
__device__ __forceinline__ void prep_cov_point(const float *raw, int ld, float res, const float *pe, const uint64_t *keys,
                                               const int32_t *hash_off, const int32_t *count, int mask, const int32_t *list, double *C) {
    const int vx = lrg_voxel_of(pe[0], res), vy = lrg_voxel_of(pe[1], res), vz = lrg_voxel_of(pe[2], res);
    double A[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, B[3] = {0, 0, 0};
    int n = 0;
    for (int dx = -1; dx <= 1; ++dx)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dz = -1; dz <= 1; ++dz) {                                 // itertools.product order (:147)
                const int slot = lrg_room_find(keys, mask, lrg_pack_voxel(vx + dx, vy + dy, vz + dz));
                if (slot < 0) continue;
                const int o = hash_off[slot], c = count[slot];
                for (int t = 0; t < c; ++t) {
                    const float *p = raw + (long)list[o + t] * ld;
                    const float x = p[0], y = p[1], z = p[2];
                    // numpy.outer(p, p) of a float32 row is float32; += into the float64 accumulator (:155)
                    A[0] += (double)__fmul_rn(x, x); A[1] += (double)__fmul_rn(x, y); A[2] += (double)__fmul_rn(x, z);
                    A[3] += (double)__fmul_rn(y, x); A[4] += (double)__fmul_rn(y, y); A[5] += (double)__fmul_rn(y, z);
                    A[6] += (double)__fmul_rn(z, x); A[7] += (double)__fmul_rn(z, y); A[8] += (double)__fmul_rn(z, z);
                    B[0] += (double)x; B[1] += (double)y; B[2] += (double)z;    // (:156)
                }
                n += c;
            }
    const double dn = (double)n, dn2 = dn * dn;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i + j] / dn - (B[i] * B[j]) / dn2;          // (:157)
}

// room extent for the normalised coordinates (:139); scal is the room's scalar block
__device__ __forceinline__ void prep_extent_point(const float *pe, int32_t *scal) {
    atomicMin(&scal[2], prep_ord(pe[0])); atomicMin(&scal[3], prep_ord(pe[1])); atomicMin(&scal[4], prep_ord(pe[2]));
    atomicMax(&scal[5], prep_ord(pe[0])); atomicMax(&scal[6], prep_ord(pe[1])); atomicMax(&scal[7], prep_ord(pe[2]));
}

// normal and curvature of one covariance (:158-161): normal [3], curv and nflag (eig_mode 2, nullable) are the point's own elements
__device__ __forceinline__ void prep_eig_point(const double *C, int eig_mode, double *normal, double *curv, int32_t *scal, int32_t *nflag) {
    double w[3], V[3][3];
    prep_jacobi3(C, w, V);
    // singular values of a symmetric matrix = |eigenvalues|, descending; V[2] belongs to the smallest (:158-159)
    double s[3] = {fabs(w[0]), fabs(w[1]), fabs(w[2])};
    int i0, i1, i2;
    prep_eig_order(s, &i0, &i1, &i2);
    normal[0] = fabs(V[i2][0]); normal[1] = fabs(V[i2][1]); normal[2] = fabs(V[i2][2]);
    const double cv = fabs(s[i2] / (s[i0] + s[i1] + s[i2]));                                         // S[2]/(S[0]+S[1]+S[2]) (:160-161)
    *curv = cv;
    if (eig_mode == 2 && nflag) {
        // Would LAPACK's decomposition of the same matrix round to the same float32 normal?  Both solvers are backward stable: their
        // eigenvectors of the smallest eigenvalue differ by at most ~p eps |A| / (gap to the next eigenvalue) with a small p; with
        // PREP_EIG_SLACK = 256 eps (an order of magnitude above either solver's constant) a component whose float32 rounding is the
        // same at both ends of that interval is the same float32 number under LAPACK.  Everything else -- near-degenerate pairs of
        // eigenvalues, components next to a rounding boundary, NaN -- is flagged and redone by the host's LAPACK call (preprocess_gpu).
        const double gap = s[i1] - s[i2];
        int unsafe = !(gap > 1e-6 * s[i0]) || !(cv == cv);
        if (!unsafe) {
            const double dv = PREP_EIG_SLACK * s[i0] / gap;
            for (int k = 0; k < 3; ++k) {
                const double x = fabs(V[i2][k]);
                if ((float)(x - dv) != (float)(x + dv) || x < dv) unsafe = 1;
            }
        }
        *nflag = unsafe;
    }
    if (cv != cv) scal[10] = 1;                                                                     // numpy's max() propagates NaN
    else atomicMax(reinterpret_cast<unsigned long long *>(&scal[8]), (unsigned long long)__double_as_longlong(cv));
}

// one row of the feature stack (:163-172): p the raw row, o the output row, normal / curv the point's own elements
__device__ __forceinline__ void prep_feature_row(const float *p, const int32_t *scal, const double *normal, double *curv, int F, float *o,
                                                 int keep_raw_curv) {
    for (int k = 0; k < 3; ++k) {
        const float mn = prep_unord(scal[2 + k]), mx = prep_unord(scal[5 + k]);
        o[k] = p[k];
        o[3 + k] = __fdiv_rn(__fsub_rn(p[k], mn), __fsub_rn(mx, mn));
    }
    if (F >= 9)
        for (int k = 0; k < 3; ++k) o[6 + k] = p[3 + k];
    if (F >= 12)
        for (int k = 0; k < 3; ++k) o[9 + k] = (float)normal[k];
    const double cmax = scal[10] ? __longlong_as_double(0x7ff8000000000000LL)
                                 : __longlong_as_double(*reinterpret_cast<const long long *>(&scal[8]));
    const double c = *curv / cmax;                                                                   // (:163)
    if (!keep_raw_curv) *curv = c;        // (eig_mode 2: the host normalises with LAPACK's own maximum)
    if (F >= 13) o[12] = (float)c;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// All rooms of a file in one pass.  The rooms' raw rows lie one after the other ([sum M, ld], room r =
// rows raw_start[r] .. raw_start[r + 1]); every kernel runs over the whole array (or over all hash slots), so the launch count does
// not depend on the number of rooms.  Room r owns a hash segment (lrg_room_hash.h): equal voxel coordinates in two rooms are keys in
// two tables and never meet.  first / list / hash_off hold file-wide raw indices; ONE scan of the first-point flags ranks the equalised points of
// all rooms back to back in room order, eq_start[r] = its value at raw_start[r]; equalized_idx / unequalized_idx are written
// room-relative.  Every room has its own status word and its own 16-word scalar block: [0] N, [1] error, [2..7] xyz min/max (ordered
// ints), [8,9] max curvature (u64), [10] any-NaN, [14,15] eq_start of a one-room call.
#define PB_SCAL 16

struct PbLayout {
    size_t keys, first, count, off, rank, cursor;     // per hash slot (all rooms' segments)
    size_t slot, flag, list, room_of, eglob;          // per raw point (eglob: per equalised point, its file-wide raw index)
    size_t rooms, status, bsum, scal, normal, curv;        // rooms: the device's raw_start
    size_t total;
    long hslots;
    int n;
};

struct PbArgs {
    const float *raw; int ld;
    const int32_t *obj, *cls; int32_t *raw_start;
    int n_rooms, n; float res; int F, eig_mode;
    uint64_t *keys; int32_t *first, *count, *off, *rank, *cursor; long hslots;
    int32_t *slot, *flag, *list, *room_of, *eglob, *bsum, *scal, *status;
    double *normal, *curv, *cov;
    float *points; int32_t *obj_out, *cls_out, *equalized_idx, *unequalized_idx, *eq_start, *unsafe;
};

// raw_start is host memory: checked here, before anything is launched
static int pb_layout(const int32_t *raw_start, int n_rooms, PbLayout *L) {
    if (n_rooms < 1 || n_rooms > (1 << 20) || !raw_start || raw_start[0] != 0) return LRG_EINVAL - 60;
    for (int r = 0; r < n_rooms; ++r) {
        if (raw_start[r + 1] < raw_start[r]) return LRG_EINVAL - 61;
        if (raw_start[r + 1] == raw_start[r]) return LRG_EINVAL - 62;              // an empty room
    }
    const long n = raw_start[n_rooms];
    if (n >= (1L << 30)) return LRG_EINVAL - 63;
    // the segments' space (an upper bound of the summed capacities): slot numbers and list offsets stay in int32
    const long hslots = lrg_room_hash_slots(n, n_rooms);
    if (hslots >= (1L << 31)) return LRG_EINVAL - 64;
    L->hslots = hslots;
    L->n = (int)n;
    LrgArena ws;
    L->keys = ws.take((size_t)hslots * 8);
    L->first = ws.take((size_t)hslots * 4);
    L->count = ws.take((size_t)hslots * 4);
    L->off = ws.take((size_t)hslots * 4);
    L->rank = ws.take((size_t)hslots * 4);
    L->cursor = ws.take((size_t)hslots * 4);
    L->slot = ws.take((size_t)n * 4);
    L->flag = ws.take((size_t)n * 4);
    L->list = ws.take((size_t)n * 4);
    L->room_of = ws.take((size_t)n * 4);
    L->eglob = ws.take((size_t)n * 4);
    L->rooms = ws.take((size_t)(n_rooms + 1) * 4);
    L->status = ws.take((size_t)n_rooms * 4);
    L->bsum = ws.take((size_t)(lrg_scan_blocks(hslots) + 1) * 4);
    L->scal = ws.take((size_t)n_rooms * PB_SCAL * 4);
    L->normal = ws.take((size_t)n * 3 * 8);
    L->curv = ws.take((size_t)n * 8);
    L->total = ws.total;
    return 0;
}

// Bounds of room r; an r out of range and an empty room are refused too
__device__ __forceinline__ bool pb_room(const PbArgs &a, int r, int *s, int *e) {
    return r >= 0 && r < a.n_rooms && lrg_room_bounds(a.raw_start, a.n, r, s, e) && *e > *s;
}

// single_n > 0: the call is one room of single_n rows, and this kernel writes its bounds to a.raw_start itself -- no copy from the
// host; with n_rooms = 1 the search below reads no bound, and every later kernel runs after this one
__global__ __launch_bounds__(PREP_THREADS) void pb_init_kernel(PbArgs a, int single_n) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (single_n > 0 && t == 0) { a.raw_start[0] = 0; a.raw_start[1] = single_n; }
    if (t < a.hslots) { a.keys[t] = LRG_HASH_EMPTY; a.first[t] = INT_MAX; a.count[t] = 0; a.cursor[t] = 0; }
    if (t < (long)a.n_rooms * PB_SCAL) {
        const int k = (int)(t % PB_SCAL);
        a.scal[t] = (k >= 2 && k <= 4) ? INT_MAX : (k >= 5 && k <= 7) ? INT_MIN : 0;
    }
    if (t < a.n_rooms) a.status[t] = 0;
    if (t < a.n) a.room_of[t] = lrg_room_of(a.raw_start, a.n_rooms, (int)t);
}

// voxel -> slot of the room's own segment (insert), first raw index and population of every voxel          (:125-133)
__global__ __launch_bounds__(PREP_THREADS) void pb_insert_kernel(PbArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int r = a.room_of[i];
    int s, e;
    a.slot[i] = -1;
    if (!pb_room(a, r, &s, &e)) return;
    const float *p = a.raw + (long)i * a.ld;
    const uint64_t key = lrg_pack_voxel(lrg_voxel_of(p[0], a.res), lrg_voxel_of(p[1], a.res), lrg_voxel_of(p[2], a.res));
    if (key == LRG_HASH_EMPTY) { a.scal[r * PB_SCAL + 1] = 1; a.status[r] = 1; return; }     // outside the 21-bit voxel window
    long off; int mask;
    lrg_room_segment(r, s, e, &off, &mask);
    const int h = lrg_room_claim(a.keys + off, mask, key);
    if (h < 0) return;
    atomicMin(&a.first[off + h], i);
    atomicAdd(&a.count[off + h], 1);
    a.slot[i] = (int)(off + h);
}

// equalised order = raw order of the first point of each voxel, rooms back to back (:127-129,:134); eq_start and the rooms' N
__global__ __launch_bounds__(PREP_THREADS) void pb_equalize_kernel(PbArgs a, const int32_t *rank_of_raw, const int32_t *bsum_total) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= a.n_rooms) {
        int s, e;
        int v = *bsum_total;
        if (i < a.n_rooms) v = pb_room(a, i, &s, &e) ? rank_of_raw[s] : 0;
        a.eq_start[i] = v;
        if (i < a.n_rooms) {
            const int nxt = i + 1 < a.n_rooms ? (pb_room(a, i + 1, &s, &e) ? rank_of_raw[s] : v) : *bsum_total;
            a.scal[i * PB_SCAL] = nxt - v;
        }
    }
    if (i >= a.n || !a.flag[i]) return;
    int s, e;
    if (!pb_room(a, a.room_of[i], &s, &e)) return;
    const int g = rank_of_raw[i];
    a.eglob[g] = i;
    a.equalized_idx[g] = i - s;
    a.rank[a.slot[i]] = g - rank_of_raw[s];
}

__global__ __launch_bounds__(PREP_THREADS) void pb_fill_kernel(PbArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int s = a.slot[i];
    if (s < 0) { a.unequalized_idx[i] = -1; return; }
    a.list[a.off[s] + atomicAdd(&a.cursor[s], 1)] = i;
    a.unequalized_idx[i] = a.rank[s];
}

__global__ __launch_bounds__(PREP_THREADS) void pb_cov_kernel(PbArgs a) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n || g >= a.eq_start[a.n_rooms]) return;
    const int i = a.eglob[g];
    if (i < 0 || i >= a.n) return;
    const int r = a.room_of[i];
    int s, e;
    if (!pb_room(a, r, &s, &e)) return;
    long off; int mask;
    lrg_room_segment(r, s, e, &off, &mask);
    const float *pe = a.raw + (long)i * a.ld;
    double C[9];
    prep_cov_point(a.raw, a.ld, a.res, pe, a.keys + off, a.off + off, a.count + off, mask, a.list, C);
    if (a.cov)
        for (int k = 0; k < 9; ++k) a.cov[(long)g * 9 + k] = C[k];
    // Every point sends min / max atomics to its room's scalars.  With a per-lane address all lanes of a room queue at the same seven
    // words (a room alone: 3x the kernel's time, profiles/prep_one_pipeline_kernels_*.csv); with a wave-uniform address the compiler
    // folds a wavefront's atomics into one each.  A wavefront lies in one room except at a room's edge: there the per-lane address.
    auto finish = [&](int32_t *scal) {
        prep_extent_point(pe, scal);
        if (a.eig_mode) prep_eig_point(C, a.eig_mode, a.normal + (long)g * 3, a.curv + g, scal, a.unsafe ? a.unsafe + g : nullptr);
    };
    const int r0 = __builtin_amdgcn_readfirstlane(r);
    if (__builtin_amdgcn_ballot_w64(r != r0) == 0) finish(a.scal + r0 * PB_SCAL);
    else finish(a.scal + r * PB_SCAL);
}

__global__ __launch_bounds__(PREP_THREADS) void pb_features_kernel(PbArgs a) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n || g >= a.eq_start[a.n_rooms]) return;
    const int i = a.eglob[g];
    if (i < 0 || i >= a.n) return;
    const int r = a.room_of[i];
    if (r < 0 || r >= a.n_rooms) return;
    prep_feature_row(a.raw + (long)i * a.ld, a.scal + r * PB_SCAL, a.normal + (long)g * 3, a.curv + g, a.F, a.points + (long)g * a.F,
                     a.eig_mode == 2 ? 1 : 0);
    if (a.obj_out) a.obj_out[g] = a.obj ? a.obj[i] : 0;
    if (a.cls_out) a.cls_out[g] = a.cls ? a.cls[i] : 0;
}

// The caller's arguments that both entries check alike
static int pb_check_modes(float resolution, int feature_size, int eig_mode, const float *points, const double *curvatures, const double *cov) {
    if (!(resolution > 0.f)) return LRG_EINVAL - 54;
    if (feature_size != 6 && feature_size != 9 && feature_size != 12 && feature_size != 13) return LRG_EINVAL - 55;
    if (eig_mode != 0 && eig_mode != 1 && eig_mode != 2) return LRG_EINVAL - 56;
    if (eig_mode >= 1 && (!points || !curvatures)) return LRG_EINVAL - 57;
    if ((eig_mode == 0 || eig_mode == 2) && !cov) return LRG_EINVAL - 58;
    return 0;
}

// The workspace's regions as kernel arguments; the entries add the caller's own pointers
static PbArgs pb_carve(const PbLayout &L, void *workspace, int n_rooms) {
    char *ws = static_cast<char *>(workspace);
    auto i32 = [&](size_t at) { return reinterpret_cast<int32_t *>(ws + at); };
    PbArgs a = {};
    a.raw_start = i32(L.rooms); a.n_rooms = n_rooms; a.n = L.n;
    a.keys = reinterpret_cast<uint64_t *>(ws + L.keys); a.first = i32(L.first); a.count = i32(L.count); a.off = i32(L.off);
    a.rank = i32(L.rank); a.cursor = i32(L.cursor); a.hslots = L.hslots;
    a.slot = i32(L.slot); a.flag = i32(L.flag); a.list = i32(L.list); a.room_of = i32(L.room_of); a.eglob = i32(L.eglob);
    a.bsum = i32(L.bsum); a.scal = i32(L.scal); a.status = i32(L.status);
    a.normal = reinterpret_cast<double *>(ws + L.normal);
    a.curv = reinterpret_cast<double *>(ws + L.curv);
    return a;
}

// The launches.  single_n = 0: a.raw_start already holds the rooms' bounds (copied on st); > 0: one room of single_n rows (pb_init_kernel)
static int pb_run(const PbLayout &L, const PbArgs &a, int single_n, hipStream_t st) {
    int rc;
    const int n = L.n;
    const long init_n = L.hslots > (long)n ? L.hslots : (long)n;            // (hslots >= 64 n_rooms covers the scalar blocks too)
    const int gi = (int)((init_n + PREP_THREADS - 1) / PREP_THREADS), gh = (int)((L.hslots + PREP_THREADS - 1) / PREP_THREADS);
    const int gm = (n + PREP_THREADS - 1) / PREP_THREADS, ge = (n + 1 + PREP_THREADS - 1) / PREP_THREADS;      // (n + 1 > n_rooms)
    hipLaunchKernelGGL(pb_init_kernel, dim3(gi), dim3(PREP_THREADS), 0, st, a, single_n);
    hipLaunchKernelGGL(pb_insert_kernel, dim3(gm), dim3(PREP_THREADS), 0, st, a);
    hipLaunchKernelGGL(prep_flag_kernel, dim3(gm), dim3(PREP_THREADS), 0, st, a.slot, a.first, n, a.flag);
    // file-wide rank of every first point (scanned into `list`, which is filled only afterwards)
    if ((rc = lrg_exscan_i32(a.flag, n, a.bsum, a.list, st))) return rc;
    hipLaunchKernelGGL(pb_equalize_kernel, dim3(ge), dim3(PREP_THREADS), 0, st, a, a.list, a.bsum + lrg_scan_blocks(n));
    if ((rc = lrg_exscan_i32(a.count, L.hslots, a.bsum, a.off, st))) return rc;
    hipLaunchKernelGGL(pb_fill_kernel, dim3(gm), dim3(PREP_THREADS), 0, st, a);
    hipLaunchKernelGGL(prep_sort_lists_kernel, dim3(gh), dim3(PREP_THREADS), 0, st, a.off, a.count, (int)L.hslots, a.list);
    hipLaunchKernelGGL(pb_cov_kernel, dim3(gm), dim3(PREP_THREADS), 0, st, a);
    if (a.eig_mode >= 1) hipLaunchKernelGGL(pb_features_kernel, dim3(gm), dim3(PREP_THREADS), 0, st, a);
    LRG_LAUNCH_CHECK();
    return 0;
}

// The one-room entries' layout: the batch's with raw_start = {0, n_raw}
static int prep_single_layout(int n_raw, PbLayout *L) {
    if (n_raw <= 0) return LRG_EINVAL - 50;
    const int32_t raw_start[2] = {0, n_raw};
    return pb_layout(raw_start, 1, L) ? LRG_EINVAL - 51 : 0;
}

extern "C" {

size_t lrg_preprocess_workspace_bytes(int n_raw) {
    PbLayout L;
    if (prep_single_layout(n_raw, &L) != 0) return 0;
    return L.total;
}

int lrg_preprocess(const float *raw, int raw_stride, const int32_t *obj_id, const int32_t *cls_id, int n_raw, float resolution,
                   int feature_size, int eig_mode, void *workspace, size_t workspace_bytes, float *points, int32_t *obj_out,
                   int32_t *cls_out, double *curvatures, int32_t *equalized_idx, int32_t *unequalized_idx, double *cov,
                   int32_t *n_equalized, void *stream) {
    PbLayout L;
    int rc = prep_single_layout(n_raw, &L);
    if (rc) return rc;
    if (!raw || raw_stride < 6 || !workspace || !equalized_idx || !unequalized_idx || !n_equalized) return LRG_EINVAL - 52;
    if (workspace_bytes < L.total || ((uintptr_t)workspace & 255)) return LRG_EINVAL - 53;
    if ((rc = pb_check_modes(resolution, feature_size, eig_mode, points, curvatures, cov))) return rc;
    hipStream_t st = (hipStream_t)stream;
    PbArgs a = pb_carve(L, workspace, 1);
    a.raw = raw; a.ld = raw_stride; a.obj = obj_id; a.cls = cls_id; a.res = resolution; a.F = feature_size; a.eig_mode = eig_mode;
    if (curvatures) a.curv = curvatures;
    a.cov = cov; a.points = points; a.obj_out = obj_out; a.cls_out = cls_out; a.equalized_idx = equalized_idx;
    a.unequalized_idx = unequalized_idx;
    a.eq_start = a.scal + PB_SCAL - 2;                  // (the two spare words at the end of the room's scalar block)
    a.unsafe = eig_mode == 2 ? a.flag : nullptr;        // (the first-point flags are read for the last time before the covariances)
    if ((rc = pb_run(L, a, n_raw, st))) return rc;
    LRG_HIP_CHECK(hipMemcpyAsync(n_equalized, a.eq_start + 1, sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    return 0;
}

/* eig_mode 2: which equalised points' float32 normals are not certain to equal LAPACK's (1) -- copied out of the workspace */
int lrg_preprocess_unsafe_normals(const void *workspace, int n_raw, int n_equalized, int32_t *flags_out, void *stream) {
    PbLayout L;
    int rc = prep_single_layout(n_raw, &L);
    if (rc) return rc;
    if (!workspace || !flags_out || n_equalized < 0 || n_equalized > n_raw) return LRG_EINVAL - 52;
    if (n_equalized == 0) return 0;
    LRG_HIP_CHECK(hipMemcpyAsync(flags_out, static_cast<const char *>(workspace) + L.flag, (size_t)n_equalized * sizeof(int32_t), hipMemcpyDeviceToDevice,
                                 (hipStream_t)stream));
    return 0;
}

/* error flag of the last lrg_preprocess on this workspace: 1 = a point fell outside the 21-bit voxel window */
int lrg_preprocess_status(const void *workspace, int n_raw, int32_t *host_status, void *stream) {
    PbLayout L;
    int rc = prep_single_layout(n_raw, &L);
    if (rc) return rc;
    if (!workspace || !host_status) return LRG_EINVAL - 52;
    LRG_HIP_CHECK(hipMemcpyAsync(host_status, static_cast<const char *>(workspace) + L.status, sizeof(int32_t), hipMemcpyDeviceToHost,
                                 (hipStream_t)stream));
    LRG_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

/* ---- all rooms of a file in one pass ---- */
size_t lrg_preprocess_batch_workspace_bytes(const int32_t *raw_start, int n_rooms) {
    PbLayout L;
    if (pb_layout(raw_start, n_rooms, &L) != 0) return 0;
    return L.total;
}

int lrg_preprocess_batch(const float *raw, int raw_stride, const int32_t *obj_id, const int32_t *cls_id, const int32_t *raw_start,
                         int n_rooms, float resolution, int feature_size, int eig_mode, void *workspace, size_t workspace_bytes,
                         float *points, int32_t *obj_out, int32_t *cls_out, double *curvatures, int32_t *equalized_idx,
                         int32_t *unequalized_idx, double *cov, int32_t *eq_start, int32_t *unsafe_flags, void *stream) {
    PbLayout L;
    int rc = pb_layout(raw_start, n_rooms, &L);
    if (rc) return rc;
    if (!raw || raw_stride < 6 || !workspace || !equalized_idx || !unequalized_idx || !eq_start) return LRG_EINVAL - 65;
    if (workspace_bytes < L.total || ((uintptr_t)workspace & 255)) return LRG_EINVAL - 66;
    if ((rc = pb_check_modes(resolution, feature_size, eig_mode, points, curvatures, cov))) return rc;
    if (eig_mode == 2 && !unsafe_flags) return LRG_EINVAL - 67;
    hipStream_t st = (hipStream_t)stream;
    PbArgs a = pb_carve(L, workspace, n_rooms);
    // a device copy of raw_start (the caller's is host memory)
    LRG_HIP_CHECK(hipMemcpyAsync(a.raw_start, raw_start, (size_t)(n_rooms + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
    a.raw = raw; a.ld = raw_stride; a.obj = obj_id; a.cls = cls_id; a.res = resolution; a.F = feature_size; a.eig_mode = eig_mode;
    if (curvatures) a.curv = curvatures;
    a.cov = cov; a.points = points; a.obj_out = obj_out; a.cls_out = cls_out; a.equalized_idx = equalized_idx;
    a.unequalized_idx = unequalized_idx; a.eq_start = eq_start; a.unsafe = eig_mode == 2 ? unsafe_flags : nullptr;
    return pb_run(L, a, 0, st);
}

/* error flags of the last lrg_preprocess_batch on this workspace, one per room: 1 = a point of the room fell outside the voxel window */
int lrg_preprocess_batch_status(const void *workspace, const int32_t *raw_start, int n_rooms, int32_t *host_status_per_room, void *stream) {
    PbLayout L;
    int rc = pb_layout(raw_start, n_rooms, &L);
    if (rc) return rc;
    if (!workspace || !host_status_per_room) return LRG_EINVAL - 65;
    LRG_HIP_CHECK(hipMemcpyAsync(host_status_per_room, static_cast<const char *>(workspace) + L.status, (size_t)n_rooms * sizeof(int32_t),
                                 hipMemcpyDeviceToHost, (hipStream_t)stream));
    LRG_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

}  // extern "C"
