// Beam-search region growing (test_beam_search.py:143-290) with the queue ON THE DEVICE; included by lrg_grow.hip.
//
// Per seed the reference keeps a queue Q of at most BEAM_WIDTH masks; every entry spawns SEARCH_WIDTH stochastic grow steps;
// the children whose mask changed are scored (--scoring np: size, ml: log-likelihood), the best BEAM_WIDTH become the next queue; the queue's
// head is the answer when its bounding box has not grown twice in a row (:188-198) or no child survives (:179).  Here a room
// in flight is a GROUP of G = BEAM_WIDTH * SEARCH_WIDTH slots -- child (qid, search id) is slot qid * SEARCH_WIDTH + search id
// -- and one level of every room in flight is one pass of the loop's kernels over all slots, bracketed by lrg_beam_advance:
// one workgroup per group that (1) turns the children's results into the next queue (stable order by score, masks copied into
// the group's parent buffers), (2) applies the stall test / commits the head / picks the next seed, (3) writes the next
// children into the slots.  Nothing returns to the host between levels; finished rooms are announced through the stats ring
// as in greedy growing.  A child's random stream is keyed (seed point, child ordinal, level), as oracle/beam_ref.py keys it.
//
// The score is the sort key of every level (:275-282).  --scoring np: the size of the child's mask.  --scoring ml (:237-257,:273):
// the parent's score plus the log-likelihood of the masks the child sampled -- lrg_beam_advance hands the parent's score to the child
// (slot.ml_score), lrg_beam_ml_score_kernel adds the child's two sides after the network has run and before lrg_mask_update moves
// slot.step on, and the next lrg_beam_advance sorts by it and keeps the survivors' scores in q_score.  The choice itself (best
// BEAM_WIDTH, stable, emptied masks dropped afterwards) is lrg_beam_select.h's, shared with a host table test.
#include "lrg_beam_select.h"

// ---- --scoring ml: the log-likelihood of the add / remove masks a child sampled at this level (test_beam_search.py:237-257) ----
// Every sample row i of a side -- padded copies included -- contributes log(conf_i) / NUM_NEIGHBOR_POINT if its un-centred,
// re-voxelised point lies in the set of voxels whose draw fired, else log(1 - conf_i) / NUM_NEIGHBOR_POINT: membership is by VOXEL,
// so a copy of a fired point counts as fired whatever its own draw said, and the remove side divides by NUM_NEIGHBOR_POINT too
// (:255,:257).  The draws are lrg_mask_update_kernel's (same keys, same policy switch), taken before it increments slot.step.
// The fired voxels go into an open-addressing LDS table of >= 2N keys (a short probe per row instead of a scan of all rows);
// float32 terms as NumPy computes them (oracle/grow_ref.py:161-170), each side summed in float64 in a fixed order -- per thread in
// row order, a shuffle tree inside the wavefront, the wavefronts in index order -- so a child's score has the same bits every run.
#define LRG_BEAM_ML_THREADS 512
#define LRG_BEAM_ML_MAXSAMPLE 1024                                   // n_inlier, n_neighbor <= 1024 (LRG_FRONT_MAXSAMPLE)
#define LRG_BEAM_ML_ROWS (LRG_BEAM_ML_MAXSAMPLE / LRG_BEAM_ML_THREADS)
__global__ __launch_bounds__(LRG_BEAM_ML_THREADS) void lrg_beam_ml_score_kernel(LrgSlot *slots, const LrgRoom *rooms, LrgGrowParams prm,
                                                                                 const float *inlier, const float *neighbor,
                                                                                 const float *center, const float *add_logits,
                                                                                 const float *rmv_logits, const int32_t *gt_remove,
                                                                                 const int32_t *gt_add, const int32_t *sample_in,
                                                                                 const int32_t *sample_nb) {
    __shared__ unsigned long long sh_tab[2 * LRG_BEAM_ML_MAXSAMPLE];
    __shared__ double sh_part[LRG_BEAM_ML_THREADS / 64];
    __shared__ double sh_side[2];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    LrgSlot *S = &slots[s];
    if (S->status != LRG_ACTIVE || S->room < 0) return;              // (idle, or a parent without neighbours: lrg_box_query stopped it)
    const LrgRoom *R = &rooms[S->room];
    const int F = prm.feature_size;
    const float res = prm.resolution;
    const float c0 = center[s * 16 + 0], c1 = center[s * 16 + 1];
    const uint32_t k0 = prm.rng_seed, k1 = (uint32_t)R->room_id;
    const uint32_t seed = (uint32_t)S->seed, restart = (uint32_t)S->restart, step = (uint32_t)S->step;
    for (int side = 0; side < 2; ++side) {                           // 0: add head on the neighbour rows, 1: remove head on the inlier rows
        const int N = side ? prm.n_inlier : prm.n_neighbor;
        const float *rows = side ? inlier : neighbor, *logits = side ? rmv_logits : add_logits;
        const int32_t *gt = side ? gt_remove : gt_add, *sample = side ? sample_in : sample_nb;
        const bool padded = sample && (side ? S->nc : S->ne) < N;    // logits exist only for the distinct leading rows then
        int T = 64;
        while (T < 2 * N) T <<= 1;                                   // table size: a power of two >= 2N (<= 2048)
        for (int i = tid; i < T; i += LRG_BEAM_ML_THREADS) sh_tab[i] = LRG_HASH_EMPTY;
        __syncthreads();
        unsigned long long key[LRG_BEAM_ML_ROWS];
        float conf[LRG_BEAM_ML_ROWS];
        bool take[LRG_BEAM_ML_ROWS];
#pragma unroll
        for (int r = 0; r < LRG_BEAM_ML_ROWS; ++r) {
            const int j = tid + r * LRG_BEAM_ML_THREADS;
            key[r] = LRG_HASH_EMPTY; conf[r] = 0.f; take[r] = false;
            if (j < N) {
                const long o = (long)s * N + j;
                const long lo = padded ? (long)s * N + sample[o] : o;
                conf[r] = lrg_conf(logits + 2 * lo);
                if (prm.policy == 2) take[r] = gt[o] != 0;
                else if (prm.policy == 1) take[r] = conf[r] > 0.5f;
                else take[r] = lrg_uniform01(lrg_rng_word((uint32_t)j, side ? LRG_PURPOSE_RMV : LRG_PURPOSE_ADD, seed, restart, step, k0, k1)) < conf[r];
                const float *p = rows + o * F;
                key[r] = lrg_pack_voxel(lrg_voxel_of(__fadd_rn(p[0], c0), res), lrg_voxel_of(__fadd_rn(p[1], c1), res), lrg_voxel_of(p[2], res));
                if (take[r] && key[r] != LRG_HASH_EMPTY) {           // (a key outside the voxel window matches nothing but itself: `take` below)
                    unsigned h = (unsigned)lrg_fmix64(key[r]) & (unsigned)(T - 1);
                    for (int probe = 0; probe < T; ++probe) {        // at most N of the T >= 2N places are ever taken: this ends
                        const unsigned long long was = atomicCAS(&sh_tab[h], LRG_HASH_EMPTY, key[r]);
                        if (was == LRG_HASH_EMPTY || was == key[r]) break;
                        h = (h + 1) & (unsigned)(T - 1);
                    }
                }
            }
        }
        __syncthreads();
        double t = 0.0;
#pragma unroll
        for (int r = 0; r < LRG_BEAM_ML_ROWS; ++r) {
            const int j = tid + r * LRG_BEAM_ML_THREADS;
            if (j < N) {
                bool in = take[r];
                if (!in && key[r] != LRG_HASH_EMPTY) {
                    unsigned h = (unsigned)lrg_fmix64(key[r]) & (unsigned)(T - 1);
                    for (int probe = 0; probe < T; ++probe) {
                        const unsigned long long k = sh_tab[h];
                        if (k == key[r]) { in = true; break; }
                        if (k == LRG_HASH_EMPTY) break;
                        h = (h + 1) & (unsigned)(T - 1);
                    }
                }
                t += (double)__fdiv_rn(in ? logf(conf[r]) : logf(__fsub_rn(1.f, conf[r])), (float)prm.n_neighbor);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
        if (lane == 0) sh_part[wave] = t;
        __syncthreads();
        if (tid == 0) {
            double sum = 0.0;
            for (int w = 0; w < LRG_BEAM_ML_THREADS / 64; ++w) sum += sh_part[w];
            sh_side[side] = sum;
        }
        __syncthreads();                                             // (sh_tab and sh_part are free for the other side)
    }
    if (tid == 0) S->ml_score = (S->ml_score + sh_side[0]) + sh_side[1];      // :273: the parent's score, plus the add side, then the remove side
}

__device__ void lrg_beam_commit(LrgBeamGroup *B, LrgRoom *R, const LrgGrowParams &prm, int64_t *stats) {
    // visited / label from the head of the queue (:289-293); workgroup-wide, ends with a barrier
    const int n = R->n;
    const int parent = B->q_parent[0];
    const int count = B->q_count[0];
    const int labeled = count > prm.cluster_threshold;
    const int cid = R->next_cluster_id;
    if (parent < 0) {
        if (threadIdx.x == 0) { R->visited[B->seed] = 1; if (labeled) R->label[B->seed] = cid; }
    } else {
        const uint8_t *mask = B->parent + (long)parent * B->cap;
        for (int i = threadIdx.x; i < n; i += blockDim.x)
            if (mask[i]) { R->visited[i] = 1; if (labeled) R->label[i] = cid; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t *log = R->region_log + LRG_LOG_WORDS * (long)R->n_regions;
        log[0] = B->seed; log[1] = B->steps; log[2] = count; log[3] = 0; log[4] = labeled; log[5] = 0; log[6] = -1; log[7] = -1;
        R->n_regions += 1;
        if (labeled) R->next_cluster_id = cid + 1;
        if (stats) atomicAdd(reinterpret_cast<unsigned long long *>(&stats[0]), 1ULL);
        B->seed = -1;
    }
    __syncthreads();
}

__global__ __launch_bounds__(1024) void lrg_beam_advance_kernel(LrgBeamGroup *groups, LrgSlot *slots, LrgRoom *rooms, int BW, int SW,
                                                                 LrgGrowParams prm, int64_t *stats) {
    __shared__ int sh_next, sh_sel[LRG_BEAM_MAXQ], sh_nsel;
    __shared__ int sh_best[LRG_BEAM_MAXQ], sh_upd[64], sh_size[64];
    __shared__ double sh_score[64];
    const int g = blockIdx.x, tid = threadIdx.x, G = BW * SW;
    const int ml = prm.scoring == 1;
    LrgBeamGroup *B = &groups[g];
    LrgSlot *S0 = &slots[g * G];
    if (B->room < 0 || B->done) {
        if (tid < G) { S0[tid].room = -1; S0[tid].status = LRG_IDLE; }
        return;
    }
    LrgRoom *R = &rooms[B->room];
    const int n = R->n;
    // ---- (1) the level just evaluated -> the next queue (:275-287) ----
    if (B->pending) {
        if (tid == 0) {
            const int nq = B->nq;
            int ran = 0;
            for (int q = 0; q < nq; ++q) ran += S0[q * SW].updated >= 0;          // a parent without neighbours spawns nothing (:212)
            B->steps += SW * ran;                                                  // :274, one per child
            // children whose mask changed, by score, ties in (qid, search id) order (a stable sort, :282); the best BW, then without
            // the emptied masks (lrg_beam_select.h)
            for (int c = 0; c < nq * SW; ++c) {
                const LrgSlot *S = &S0[c];
                sh_upd[c] = S->updated; sh_size[c] = S->scan_cnt;
                sh_score[c] = ml ? S->ml_score : (double)S->scan_cnt;
            }
            int nb = 0;
            sh_nsel = lrg_beam_select(nq * SW, sh_upd, sh_size, sh_score, ml, BW, sh_best, &nb, sh_sel);
            if (B->trace && B->trace_count) {                                      // what was chosen, for a checker that follows the search
                const int at = atomicAdd(B->trace_count, 1);
                if (at < B->trace_cap) {
                    LrgBeamTraceRec *T = &B->trace[at];
                    T->room = B->room; T->seed = B->seed; T->level = B->level; T->n = nb;
                    for (int k = 0; k < LRG_BEAM_MAXQ; ++k) {
                        const int c = k < nb ? sh_best[k] : -1;
                        T->ordinal[k] = c; T->size[k] = c < 0 ? 0 : sh_size[c]; T->score[k] = c < 0 ? 0.0 : sh_score[c];
                    }
                }
            }
        }
        __syncthreads();
        const int ns = sh_nsel;
        if (ns == 0) {
            lrg_beam_commit(B, R, prm, stats);             // the queue ran dry: its last head is the answer (:179,:289)
        } else {
            for (int k = 0; k < ns; ++k) {                  // the survivors' masks become the parents of the next level
                const uint8_t *src = S0[sh_sel[k]].cur;
                uint8_t *dst = B->parent + (long)k * B->cap;
                for (int i = tid; i < n; i += blockDim.x) dst[i] = src[i];
            }
            __syncthreads();
            if (tid == 0) {
                for (int k = 0; k < ns; ++k) {
                    const LrgSlot *S = &S0[sh_sel[k]];
                    B->q_count[k] = S->scan_cnt; B->q_parent[k] = k; B->q_score[k] = ml ? S->ml_score : 0.0;
                    for (int d = 0; d < 3; ++d) { B->q_mn[k][d] = S->scan_mn[d]; B->q_mx[k][d] = S->scan_mx[d]; }
                }
                B->nq = ns;
                B->level += 1;
            }
            __syncthreads();
        }
        if (tid == 0) B->pending = 0;
        __syncthreads();
    }
    // ---- (2) stall test on the head (:188-198), commit, next seed (:154-174) ----
    for (;;) {
        if (B->seed < 0) {
            int cursor = R->seed_cursor, found = -1;
            while (cursor < n) {
                const int pos = cursor + tid;
                int cand = INT_MAX;
                if (pos < n && !R->visited[R->order[pos]]) cand = pos;
                if (tid == 0) sh_next = INT_MAX;
                __syncthreads();
                if (cand != INT_MAX) atomicMin(&sh_next, cand);
                __syncthreads();
                const int best = sh_next;
                __syncthreads();
                if (best != INT_MAX) { found = best; break; }
                cursor += blockDim.x;
            }
            if (found < 0) {
                if (tid == 0) {
                    R->seed_cursor = n; R->done = 1; B->done = 1;
                    if (stats) {
                        unsigned long long k = atomicAdd(reinterpret_cast<unsigned long long *>(&stats[1]), 1ULL);
                        stats[4 + (k % LRG_DONE_RING)] = g * G;
                    }
                }
                if (tid < G) { S0[tid].room = -1; S0[tid].status = LRG_IDLE; }
                return;
            }
            if (tid == 0) {
                const int sd = R->order[found];
                R->seed_cursor = found + 1;
                B->seed = sd; B->level = 0; B->stuck = 0; B->steps = 0; B->nq = 1;
                B->q_count[0] = 1; B->q_parent[0] = -1; B->q_score[0] = 0.0;     // the seed-only mask, score 0 (:164-174)
                for (int d = 0; d < 3; ++d) {
                    const int v = R->voxels[3 * sd + d];
                    B->q_mn[0][d] = v; B->q_mx[0][d] = v; B->seq_mn[d] = v; B->seq_mx[d] = v;
                }
            }
            __syncthreads();
        }
        bool commit = false;
        if (tid == 0) {
            bool grew = false;
            for (int d = 0; d < 3; ++d) grew |= B->q_mn[0][d] < B->seq_mn[d] || B->q_mx[0][d] > B->seq_mx[d];
            if (!grew) {
                if (B->stuck >= 1) sh_next = 1; else { B->stuck += 1; sh_next = 0; }
            } else { B->stuck = 0; sh_next = 0; }
            if (!sh_next)
                for (int d = 0; d < 3; ++d) { B->seq_mn[d] = min(B->seq_mn[d], B->q_mn[0][d]); B->seq_mx[d] = max(B->seq_mx[d], B->q_mx[0][d]); }
        }
        __syncthreads();
        commit = sh_next != 0;
        __syncthreads();
        if (!commit) break;
        lrg_beam_commit(B, R, prm, stats);
    }
    // ---- (3) the children of this level ----
    const int nq = B->nq, seed = B->seed;
    for (int c = 0; c < nq * SW; ++c) {
        const int q = c / SW;
        uint8_t *dst = S0[c].cur;
        const int parent = B->q_parent[q];
        if (parent < 0) { for (int i = tid; i < n; i += blockDim.x) dst[i] = i == seed; }
        else {
            const uint8_t *src = B->parent + (long)parent * B->cap;
            for (int i = tid; i < n; i += blockDim.x) dst[i] = src[i];
        }
    }
    if (tid < G) {
        LrgSlot *S = &S0[tid];
        if (tid < nq * SW) {
            const int q = tid / SW;
            S->room = B->room; S->status = LRG_ACTIVE; S->seed = seed; S->step = B->level; S->restart = tid;   // RNG key: (seed, ordinal, level)
            S->steps_total = 0; S->stuck = 0; S->pad = 0; S->nc = 0; S->ne = 0; S->query = 0; S->scan_cnt = 0; S->updated = -1;
            S->count = B->q_count[q];
            S->ml_score = B->q_score[q];                                            // the parent's score (:273 adds the child's sides to it)
            S->target = R->obj_id ? R->obj_id[seed] : 0;
            for (int d = 0; d < 3; ++d) {
                S->mn[d] = B->q_mn[q][d]; S->mx[d] = B->q_mx[q][d];
                S->scan_mn[d] = INT_MAX; S->scan_mx[d] = INT_MIN;
            }
        } else { S->room = -1; S->status = LRG_IDLE; }
    }
    if (tid == 0) B->pending = 1;
}
