// Growth trace and frame renderer of animate_region_growing.py (include/lrg_hip.h: lrg_trace_snapshot, lrg_render_visibility,
// lrg_render_shade).  Everything here READS the grower's buffers (LrgSlot, LrgRoom, masks, lists, region log) and writes buffers of its
// own: the front, tile and update kernels are untouched.
//
// Trace.  After a packed iteration an ACTIVE slot stands between evaluation and mask update: snapshot k fixes step k's `before`
// (the slot's mask) and `neighbour` (its candidate list) sets, snapshot k + 1 completes its `after` set -- the slot's mask while it is
// still on the same seed one step on, else the points that became visited since snapshot k minus the seeds of the zero-step
// 'noneighbor' regions logged behind the finished one (currentMask is disjoint from visited, :318-320, so that difference is exact).
// Two launches per snapshot: the PLAN kernel decides from the slot, the room and the trace's state words what this snapshot finishes
// and starts, writes that decision (plan words, the new frame's header) and scatters the two lists into a mark byte per point; the
// POINT kernel then walks the points once with everything it needs beside it.  No block of either launch reads a word another block
// of the same launch writes: the state words are read by the plan kernel and written by the point kernel.
#include "lrg_common.h"

#define TRACE_THREADS 256
#define TRACE_PLAN_BLOCKS 32
// state words
enum { TS_FRAMES = 0, TS_PENDING = 1, TS_NREG = 2, TS_ERROR = 3, TS_DONE = 4 };
// plan words
enum { TP_MODE = 0, TP_FIN = 1, TP_START = 2, TP_NEW = 3, TP_COLOUR = 4, TP_NREG = 5, TP_ERROR = 6 };
// header words: seed, 1-based step, next_cluster_id, inlier, neighbour, add, remove, 1 once `after` is in
enum { TH_SEED = 0, TH_STEP = 1, TH_CID = 2, TH_INLIER = 3, TH_NEIGHBOR = 4, TH_ADD = 5, TH_REMOVE = 6, TH_COMPLETE = 7 };
#define MARK_SEED 1
#define MARK_NEIGHBOR 2

struct TraceArgs {
    const LrgSlot *slots; const LrgRoom *rooms;
    int slot, room, n, stride, cap_frames, consumed;
    int32_t *state, *plan, *headers;
    uint8_t *codes, *paints, *paint, *vis_prev, *mark;
    const int32_t *mult;
};

struct TracePlan { int mode, fin, start, fresh, colour, nreg, error, rows_lo, rows_hi, ne; };

// The decision of one snapshot, from words no block of the plan launch writes (uniform over the launch)
__device__ __forceinline__ TracePlan trace_decide(const TraceArgs &a) {
    TracePlan p = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const LrgSlot *S = a.slots + a.slot;
    const LrgRoom *R = a.rooms + a.room;
    const int frames = a.state[TS_FRAMES], pending = a.state[TS_PENDING], nreg_prev = a.state[TS_NREG];
    const int nreg = R->n_regions;
    p.nreg = nreg;
    if (R->n != a.n || frames < 0 || nreg < 0 || nreg > a.n) { p.error = 8; return p; }      // not the room the buffers were sized for
    const bool active = S->status == LRG_ACTIVE && S->room == a.room;
    bool open = pending != 0;
    if (pending) {
        const int f = (frames - 1) % a.cap_frames;
        const int32_t *h = a.headers + 8 * f;
        if (active && S->seed == h[TH_SEED] && S->step == h[TH_STEP] && nreg == nreg_prev) p.mode = 1;
        else if (nreg > nreg_prev) { p.mode = 2; p.rows_lo = nreg_prev + 1; p.rows_hi = nreg; }
        else if (active) p.error = 1;               // a step nobody finished: the slot moved on without a region being logged
        if (p.mode) {
            p.fin = f;
            p.colour = ((h[TH_CID] - 1) % 19 + 19) % 19 + 1;
            open = false;
        }
    }
    if (active && !open && !p.error) {
        if (frames - a.consumed >= a.cap_frames) p.error = 4;      // the host has not taken the frames of the ring yet
        else { p.start = 1; p.fresh = frames % a.cap_frames; p.ne = min(max(S->ne, 0), a.n); }
    }
    return p;
}

__global__ __launch_bounds__(TRACE_THREADS) void lrg_trace_plan_kernel(TraceArgs a) {
    const TracePlan p = trace_decide(a);
    const LrgSlot *S = a.slots + a.slot;
    const LrgRoom *R = a.rooms + a.room;
    const int tid = blockIdx.x * TRACE_THREADS + threadIdx.x, nth = gridDim.x * TRACE_THREADS;
    if (tid == 0) {
        a.plan[TP_MODE] = p.mode; a.plan[TP_FIN] = p.fin; a.plan[TP_START] = p.start; a.plan[TP_NEW] = p.fresh;
        a.plan[TP_COLOUR] = p.colour; a.plan[TP_NREG] = p.nreg; a.plan[TP_ERROR] = p.error;
        if (p.start) {
            int32_t *h = a.headers + 8 * p.fresh;
            h[TH_SEED] = S->seed; h[TH_STEP] = S->step + 1; h[TH_CID] = R->next_cluster_id;
            h[TH_INLIER] = 0; h[TH_NEIGHBOR] = 0; h[TH_ADD] = 0; h[TH_REMOVE] = 0; h[TH_COMPLETE] = 0;
        }
    }
    int bad = 0;
    if (p.mode == 2) {      // the seeds of the zero-step regions logged behind the finished one
        const int32_t *log = R->region_log;
        for (int r = p.rows_lo + tid; r < p.rows_hi; r += nth) {
            const int sd = log[LRG_LOG_WORDS * (long)r];
            if (sd >= 0 && sd < a.n) atomicOr(reinterpret_cast<unsigned *>(a.mark + (sd & ~3)), (unsigned)MARK_SEED << (8 * (sd & 3))); else bad = 1;
        }
    }
    if (p.start) {          // the candidates of the step evaluated in this call (:318-320): distinct points in index order
        const int32_t *cand = S->cand_idx;
        for (int k = tid; k < p.ne; k += nth) {
            const int id = cand[k];
            if (id >= 0 && id < a.n) atomicOr(reinterpret_cast<unsigned *>(a.mark + (id & ~3)), (unsigned)MARK_NEIGHBOR << (8 * (id & 3))); else bad = 1;
        }
    }
    if (bad) atomicOr(&a.plan[TP_ERROR + 1], 2);
}

// four points per thread: the grower's masks and flags start 16-byte aligned (LrgRoom.pvox) and the trace's own rows are `stride` apart
__global__ __launch_bounds__(TRACE_THREADS) void lrg_trace_point_kernel(TraceArgs a) {
    const int mode = a.plan[TP_MODE], start = a.plan[TP_START];
    const LrgSlot *S = a.slots + a.slot;
    const LrgRoom *R = a.rooms + a.room;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int err = a.plan[TP_ERROR] | a.plan[TP_ERROR + 1];
        a.plan[TP_ERROR + 1] = 0;
        if (err) a.state[TS_ERROR] |= err;
        if (mode) { a.headers[8 * a.plan[TP_FIN] + TH_COMPLETE] = 1; a.state[TS_PENDING] = 0; a.state[TS_DONE] += 1; }
        if (start) { a.state[TS_FRAMES] += 1; a.state[TS_PENDING] = 1; a.state[TS_NREG] = a.plan[TP_NREG]; }
    }
    if (!mode && !start) return;
    const uint8_t *cur = S->cur, *visited = R->visited;
    uint8_t *codeF = a.codes + (long)a.plan[TP_FIN] * a.stride, *paintF = a.paints + (long)a.plan[TP_FIN] * a.stride;
    uint8_t *codeN = a.codes + (long)a.plan[TP_NEW] * a.stride;
    const int colour = a.plan[TP_COLOUR];
    int c_in = 0, c_nb = 0, c_add = 0, c_rmv = 0;
    const int words = (a.n + 3) >> 2;
    for (int w = blockIdx.x * TRACE_THREADS + threadIdx.x; w < words; w += gridDim.x * TRACE_THREADS) {
        const int i0 = 4 * w;
        const unsigned live = i0 + 4 <= a.n ? 0xffffffffu : (0xffffffffu >> (8 * (i0 + 4 - a.n)));
        // (nonzero bytes -> 0x01 per byte)
        unsigned cw = *reinterpret_cast<const unsigned *>(cur + i0), vw = *reinterpret_cast<const unsigned *>(visited + i0);
        unsigned mk = *reinterpret_cast<const unsigned *>(a.mark + i0);
        cw = ((cw | (cw >> 1) | (cw >> 2) | (cw >> 3) | (cw >> 4) | (cw >> 5) | (cw >> 6) | (cw >> 7)) & 0x01010101u) & live;
        vw = ((vw | (vw >> 1) | (vw >> 2) | (vw >> 3) | (vw >> 4) | (vw >> 5) | (vw >> 6) | (vw >> 7)) & 0x01010101u) & live;
        int4 m = make_int4(0, 0, 0, 0);
        if (cw | vw | mk) m = *reinterpret_cast<const int4 *>(a.mult + i0);      // (mult is padded to `stride` words)
        const int mm[4] = {m.x, m.y, m.z, m.w};
        if (mode) {
            const unsigned code = *reinterpret_cast<const unsigned *>(codeF + i0), before = code & 0x01010101u;
            unsigned after;
            if (mode == 1) after = cw;
            else after = vw & ~*reinterpret_cast<const unsigned *>(a.vis_prev + i0) & ~(mk & 0x01010101u) & 0x01010101u;
            *reinterpret_cast<unsigned *>(codeF + i0) = code | (after << 2);
            unsigned pw = *reinterpret_cast<const unsigned *>(a.paint + i0);
            if (after) {
                const unsigned sel = after * 0xffu;
                pw = (pw & ~sel) | ((unsigned)colour * after);
                *reinterpret_cast<unsigned *>(a.paint + i0) = pw;
            }
            *reinterpret_cast<unsigned *>(paintF + i0) = pw;
            const unsigned add = after & ~before, rmv = before & ~after;
            if (add | rmv) {
#pragma unroll
                for (int k = 0; k < 4; ++k) { c_add += (add >> (8 * k) & 1) ? mm[k] : 0; c_rmv += (rmv >> (8 * k) & 1) ? mm[k] : 0; }
            }
        }
        if (start) {
            const unsigned nb = (mk >> 1) & 0x01010101u & live;
            *reinterpret_cast<unsigned *>(codeN + i0) = cw | (nb << 1);
            *reinterpret_cast<unsigned *>(a.vis_prev + i0) = vw;
            if (cw | nb) {
#pragma unroll
                for (int k = 0; k < 4; ++k) { c_in += (cw >> (8 * k) & 1) ? mm[k] : 0; c_nb += (nb >> (8 * k) & 1) ? mm[k] : 0; }
            }
        }
        if (mk) *reinterpret_cast<unsigned *>(a.mark + i0) = 0;      // the marks are this snapshot's alone
    }
    c_in = lrg_wave_sum_i32(c_in); c_nb = lrg_wave_sum_i32(c_nb); c_add = lrg_wave_sum_i32(c_add); c_rmv = lrg_wave_sum_i32(c_rmv);
    if (lrg_lane() == 0) {
        if (c_in) atomicAdd(a.headers + 8 * a.plan[TP_NEW] + TH_INLIER, c_in);
        if (c_nb) atomicAdd(a.headers + 8 * a.plan[TP_NEW] + TH_NEIGHBOR, c_nb);
        if (c_add) atomicAdd(a.headers + 8 * a.plan[TP_FIN] + TH_ADD, c_add);
        if (c_rmv) atomicAdd(a.headers + 8 * a.plan[TP_FIN] + TH_REMOVE, c_rmv);
    }
}

extern "C" int lrg_trace_snapshot(const LrgSlot *slots, const LrgRoom *rooms, int slot, int room, int n, int stride, int cap_frames,
                                  int consumed, int32_t *state, int32_t *plan, int32_t *headers, uint8_t *codes, uint8_t *paints,
                                  uint8_t *paint, uint8_t *vis_prev, uint8_t *mark, const int32_t *mult, void *stream) {
    if (!slots || !rooms || !state || !plan || !headers || !codes || !paints || !paint || !vis_prev || !mark || !mult) return LRG_EINVAL;
    if (slot < 0 || room < 0 || n < 1 || stride < n || stride % 16 || cap_frames < 2 || consumed < 0) return LRG_EINVAL;
    for (const void *p : {(const void *)codes, (const void *)paints, (const void *)paint, (const void *)vis_prev, (const void *)mark, (const void *)mult})
        if ((uintptr_t)p % 16) return LRG_EINVAL;
    TraceArgs a = {slots, rooms, slot, room, n, stride, cap_frames, consumed, state, plan, headers, codes, paints, paint, vis_prev, mark, mult};
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(lrg_trace_plan_kernel, dim3(TRACE_PLAN_BLOCKS), dim3(TRACE_THREADS), 0, st, a);
    const int words = (n + 3) / 4;
    hipLaunchKernelGGL(lrg_trace_point_kernel, dim3(min(1024, (words + TRACE_THREADS - 1) / TRACE_THREADS)), dim3(TRACE_THREADS), 0, st, a);
    LRG_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Renderer: every frame draws the same raw points from the same camera (animate_region_growing.py:165-182), only the colours
// change -- so the points are rasterised once into a visibility buffer and every frame is a look-up through it.
// ---------------------------------------------------------------------------------------------------------------------------
struct Mat4 { float m[16]; };

// GL_POINTS of glPointSize(size) under GL_DEPTH_TEST / GL_LESS, first drawn wins (:171-179): the smallest (depth bits, raw index) key per pixel
__global__ __launch_bounds__(256) void lrg_render_visibility_kernel(const float *xyz, int M, Mat4 mat, int W, int H, int half,
                                                                    unsigned long long *vis) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const float x = xyz[3 * (long)j], y = xyz[3 * (long)j + 1], z = xyz[3 * (long)j + 2];
    const float *m = mat.m;
    const float cx = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
    const float cy = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
    const float cz = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
    const float cw = ((m[12] * x + m[13] * y) + m[14] * z) + m[15];
    // (written so that a NaN fails every test)
    if (!(cw > 0.0f && -cw <= cx && cx <= cw && -cw <= cy && cy <= cw && -cw <= cz && cz <= cw)) return;
    const float nx = __fdiv_rn(cx, cw), ny = __fdiv_rn(cy, cw), nz = __fdiv_rn(cz, cw);
    const float xw = (nx * 0.5f + 0.5f) * (float)W, yw = (ny * 0.5f + 0.5f) * (float)H;
    const float depth = nz * 0.5f + 0.5f;
    if (!(xw >= 0.0f && xw <= (float)W && yw >= 0.0f && yw <= (float)H)) return;      // (|ndc| <= 1 puts every finite point inside; inf / inf does not pass)
    const int ix = (int)floorf(xw), iy = (int)floorf(yw);
    const unsigned long long key = ((unsigned long long)__float_as_uint(depth) << 32) | (unsigned)j;
    const int x0 = max(ix - half, 0), x1 = min(ix + half, W - 1), y0 = max(iy - half, 0), y1 = min(iy + half, H - 1);
    for (int py = y0; py <= y1; ++py) {
        unsigned long long *row = vis + (long)(H - 1 - py) * W;
        for (int px = x0; px <= x1; ++px)
            if (row[px] > key) atomicMin(row + px, key);      // (a stale plain load only costs an atomic that loses)
    }
}

extern "C" int lrg_render_visibility(const float *xyz, int M, const float *matrix_host, int W, int H, int point_size,
                                     unsigned long long *vis, void *stream) {
    if (!xyz || !matrix_host || !vis || M < 0 || W < 1 || H < 1 || (long)W * H > INT_MAX) return LRG_EINVAL;
    if (point_size < 1 || point_size > 63 || point_size % 2 == 0) return LRG_EINVAL - 1;      // odd sizes: a square centred on the pixel
    hipStream_t st = (hipStream_t)stream;
    LRG_HIP_CHECK(hipMemsetAsync(vis, 0xff, sizeof(unsigned long long) * (size_t)W * H, st));
    if (M == 0) return 0;
    Mat4 mat;
    for (int k = 0; k < 16; ++k) mat.m[k] = matrix_host[k];
    hipLaunchKernelGGL(lrg_render_visibility_kernel, dim3((M + 255) / 256), dim3(256), 0, st, xyz, M, mat, W, H, (point_size - 1) / 2, vis);
    LRG_LAUNCH_CHECK();
    return 0;
}

#define RENDER_TEXT_LINES 5
struct ShadeArgs {
    const unsigned long long *vis; const int32_t *uneq; int M, n, W, H, T;
    const uint8_t *index; long index_stride; const uint8_t *luts; const int32_t *frame_lut; int n_luts;
    const uint8_t *text; int text_len; const uint8_t *font; int font_first, font_count, scale, text_x, white;
    int text_y[RENDER_TEXT_LINES];
    uint8_t *out;
};

// 1 if pixel (px, py) of frame t lies on a glyph stroke: glyph cells of 6 x 8 font pixels (5 x 7 drawn), `scale` screen pixels each
__device__ __forceinline__ int shade_text_hit(const ShadeArgs &a, int t, int px, int py) {
    const int cx = px - a.text_x;
    if (cx < 0) return 0;
    const int cell = 6 * a.scale, ci = cx / cell, col = (cx - ci * cell) / a.scale;
    if (ci >= a.text_len || col >= 5) return 0;
    for (int k = 0; k < RENDER_TEXT_LINES; ++k) {
        const int ly = py - a.text_y[k];
        if (ly < 0 || ly >= 7 * a.scale) continue;
        const int ch = a.text[((long)t * RENDER_TEXT_LINES + k) * a.text_len + ci] - a.font_first;
        if (ch < 0 || ch >= a.font_count) continue;
        if (a.font[7 * ch + ly / a.scale] >> (4 - col) & 1) return 1;
    }
    return 0;
}

// VEC pixels of one image row per thread, all T frames: the visibility words and the raw -> equalised look-ups are read once
template <int VEC>
__global__ __launch_bounds__(256) void lrg_render_shade_kernel(ShadeArgs a) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    const int per_row = a.W / VEC;
    if (g >= (long)per_row * a.H) return;
    const int py = (int)(g / per_row), px0 = (int)(g % per_row) * VEC;
    int pt[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        const unsigned long long v = a.vis[(long)py * a.W + px0 + k];
        const unsigned raw = (unsigned)(v & 0xffffffffULL);
        int e = -1;
        if (v != ~0ULL && raw < (unsigned)a.M) { e = a.uneq[raw]; if (e < 0 || e >= a.n) e = -1; }
        pt[k] = e;
    }
    const int in_text = a.text != nullptr && py >= a.text_y[0] && py < a.text_y[RENDER_TEXT_LINES - 1] + 7 * a.scale && px0 + VEC > a.text_x;
    for (int t = 0; t < a.T; ++t) {
        const uint8_t *idx = a.index + t * a.index_stride;
        const int l = a.frame_lut[t];
        const uint8_t *lut = a.luts + 256 * (l >= 0 && l < a.n_luts ? l : 0);
        unsigned word = 0;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            unsigned v = pt[k] >= 0 ? lut[idx[pt[k]]] : 0;
            if (in_text && shade_text_hit(a, t, px0 + k, py)) v = (unsigned)a.white;
            word |= v << (8 * k);
        }
        uint8_t *dst = a.out + ((long)t * a.H + py) * a.W + px0;
        if (VEC == 4) *reinterpret_cast<unsigned *>(dst) = word; else *dst = (uint8_t)word;
    }
}

extern "C" int lrg_render_shade(const unsigned long long *vis, const int32_t *unequalized_idx, int M, int n, int W, int H, int T,
                                const uint8_t *index, long index_stride, const uint8_t *luts, int n_luts, const int32_t *frame_lut,
                                const uint8_t *text, int text_len, const uint8_t *font, int font_first, int font_count, int white,
                                uint8_t *out, void *stream) {
    if (!vis || !unequalized_idx || !index || !luts || !frame_lut || !out) return LRG_EINVAL;
    if (M < 0 || n < 1 || W < 1 || H < 1 || (long)W * H > INT_MAX || T < 0 || index_stride < n || n_luts < 1 || white < 0 || white > 255) return LRG_EINVAL;
    if (text && (!font || text_len < 1 || font_count < 1)) return LRG_EINVAL;
    if (T == 0) return 0;
    ShadeArgs a;
    a.vis = vis; a.uneq = unequalized_idx; a.M = M; a.n = n; a.W = W; a.H = H; a.T = T;
    a.index = index; a.index_stride = index_stride; a.luts = luts; a.frame_lut = frame_lut; a.n_luts = n_luts;
    a.text = text; a.text_len = text_len; a.font = font; a.font_first = font_first; a.font_count = font_count; a.white = white;
    // the reference's 40-pixel font and its lines at (10, 10 + 50 k) of a 1000-pixel window (:396-401), scaled by H / 1000
    a.scale = max(1, 40 * H / 8000);
    a.text_x = 10 * H / 1000;
    for (int k = 0; k < RENDER_TEXT_LINES; ++k) a.text_y[k] = (10 + 50 * k) * H / 1000;
    a.out = out;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = W % 4 == 0 && (uintptr_t)out % 4 == 0;
    const long threads = (long)(vec ? W / 4 : W) * H;
    if (vec) hipLaunchKernelGGL(lrg_render_shade_kernel<4>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(lrg_render_shade_kernel<1>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, a);
    LRG_LAUNCH_CHECK();
    return 0;
}
