/* lrg_hip.h -- C-ABI of liblrg_hip.so: the MI355X (gfx950) LRGNet region-grow hot path.
 *
 * Conventions (all entry points):
 *   - pointers are DEVICE pointers unless a parameter is documented as host; buffers are caller-owned;
 *   - tensors are dense row-major; kernels of the network are [Cin,Cout] row-major, i.e. the TF
 *     variable of shape [1,Cin,Cout] (learn_region_grow_util.py:107) with the leading 1 dropped;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the null stream) and the
 *     call returns without synchronising; no entry point allocates or frees device memory;
 *   - return value: 0 on success, -(hipError_t) on a HIP failure, LRG_EINVAL (-1000 - n) on a bad
 *     argument; re-entrant, no global state.
 *
 * Every entry point names the reference interface it replaces (file:line under the reference repo).
 */
#ifndef LRG_HIP_H
#define LRG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LRG_ABI_VERSION 26
#define LRG_EINVAL (-1000)
#define LRG_ERESIDENCY (-1100)  /* lrg_grow_async: the launch's workgroups cannot all be resident at once on this stream / device (see there) */

#define LRG_MAX_CONV 5 /* branch layers: lite=0 -> 5, lite=1 -> 2, lite=2 -> 3  (learn_region_grow_util.py:77-85) */
#define LRG_MAX_HEAD 3 /* head layers incl. the final 2-wide one: lite=0 -> 3, lite=1 -> 2, lite=2 -> 3        */

int lrg_abi_version(void);
/* Name of the code object's target ("gfx950"); a build sanity hook for the loader. */
const char *lrg_target_arch(void);
/* sizeof() of the ABI structs as compiled (0 LrgWeights, 1 LrgRoom, 2 LrgSlot, 3 LrgGrowParams, 4 LrgStepBuffers, 5 LrgPackedBuffers, 6 LrgBeamGroup, 7 LrgAsyncBuffers, 8 LrgFillJob), so that a
 * foreign-language binding can verify its mirror of the layout at load time. */
size_t lrg_struct_size(int which);

/* ------------------------------------------------------------------------------------------------
 * LrgNet forward   (replaces: sess.run([net.add_output, net.remove_output], ...) at
 * test_region_grow.py:257-258 on the graph built by learn_region_grow_util.py:75-162)
 * ---------------------------------------------------------------------------------------------- */
typedef struct LrgWeights {
    int32_t feature_size;            /* F: 13 (6/9/12 variants, test_region_grow.py:72-77)                 */
    int32_t n_conv;                  /* branch layers                                                       */
    int32_t n_head;                  /* head layers including the final [C,2] layer                         */
    int32_t reserved;
    int32_t conv_ch[LRG_MAX_CONV];   /* CONV_CHANNELS                                                       */
    int32_t head_ch[LRG_MAX_HEAD];   /* CONV2_CHANNELS followed by 2                                        */
    const float *inlier_w[LRG_MAX_CONV];   /* lrg_kernel{i}          [Cin,Cout]   :107                      */
    const float *inlier_b[LRG_MAX_CONV];   /* lrg_bias{i}            [Cout]       :108                      */
    const float *neighbor_w[LRG_MAX_CONV]; /* lrg_neighbor_kernel{i}              :115                      */
    const float *neighbor_b[LRG_MAX_CONV]; /* lrg_neighbor_bias{i}                :116                      */
    const float *add_w[LRG_MAX_HEAD];      /* lrg_add_kernel{j}; j=0 is [2*C_last + conv_ch[1], C]  :139,:145 */
    const float *add_b[LRG_MAX_HEAD];      /* lrg_add_bias{j}                                       :140,:146 */
    const float *rmv_w[LRG_MAX_HEAD];      /* lrg_remove_kernel{j}                                  :152,:158 */
    const float *rmv_b[LRG_MAX_HEAD];      /* lrg_remove_bias{j}                                    :153,:159 */
    const void *packed;                    /* nullable: lrg_pack_weights() image of the kernels above (MFMA operand order).
                                              NULL: lrg_forward (LRG_FWD_FUSED) re-packs into its workspace on every call,
                                              which is always correct; non-NULL: the caller vouches it is current.   */
} LrgWeights;

/* The fused kernels read the [Cin,Cout] kernels in the order their MFMA B operands want them (one 16-byte load per lane
 * per 8 rows of Cin instead of four strided 4-byte loads).  lrg_pack_weights writes that image (device memory,
 * lrg_packed_weights_bytes(w) bytes, 256-byte aligned) from the TF-layout pointers in `w`; store its address in
 * w->packed after a restore (test_region_grow.py:92-93) and repeat after any change of the variables. */
size_t lrg_packed_weights_bytes(const LrgWeights *w);
int lrg_pack_weights(const LrgWeights *w, void *packed, size_t packed_bytes, void *stream);

#define LRG_FWD_FUSE_POOL 1u /* layer-streamed path: fold the max-pool (:122-123) into the last branch layer's epilogue */
#define LRG_FWD_FUSED 2u     /* whole branch / whole head per 64-row tile in one kernel each: activations stay in LDS,
                                only conv[1], the pooled maxima and the logits reach HBM (3 launches per call)         */
#define LRG_FWD_KEEP_ACTS 4u /* with LRG_FWD_FUSED: also copy every intermediate into the workspace (parity tests)     */
#define LRG_FWD_TILE_LISTS 16u /* lrg_forward_rows + LRG_FWD_FUSED: the workspace's tile-list block (view kind 6) was filled by
                                  lrg_prepare for exactly these row counts: only the listed 32-row tiles are launched as
                                  working workgroups, back to back, so they spread evenly over the compute units (skipping
                                  by row count alone leaves the survivors wherever the dead tiles happened to sit).      */
#define LRG_ROW_TILE 32        /* rows per tile of those lists */
#define LRG_FWD_STREAM_TILES 32u /* layer-streamed path (no LRG_FWD_FUSED): every layer launch runs on the fused stacks' tile (a 1-layer stack: input rows staged once
                                 for all column blocks, weights in operand order, output from the accumulators to HBM) instead of lrg_pointwise_mfma_kernel's
                                 64 x 64 tiles; same layer-by-layer formulation and HBM traffic model (ABI 9)                                                     */
#define LRG_FWD_POOL_ZEROED 8u /* with LRG_FWD_FUSED: the workspace was zero-filled once by the caller and is only ever used
                                by calls carrying this flag -- the pooled-feature block is then zero on entry and is
                                left zero on return (cleared by the head kernel), which saves the per-call memset.
                                Precondition on rows: rows_nb[b] > 0 whenever rows_in[b] > 0.                            */

/* Bytes of scratch lrg_forward needs for a batch of B instances (host-side arithmetic only). */
size_t lrg_forward_workspace_bytes(const LrgWeights *w, int B, int n_inlier, int n_neighbor);

/* inlier [B,n_inlier,F], neighbor [B,n_neighbor,F] -> add_logits [B,n_neighbor,2] (net.add_output :149),
 * rmv_logits [B,n_inlier,2] (net.remove_output :162).  `w` is a HOST struct holding device pointers. */
int lrg_forward(const LrgWeights *w, const float *inlier, const float *neighbor, int B, int n_inlier,
                int n_neighbor, float *add_logits, float *rmv_logits, void *workspace, size_t workspace_bytes,
                unsigned flags, void *stream);

/* lrg_forward restricted to the leading rows of each instance.  rows_in / rows_nb ([B] device int32, both or
 * neither NULL): only rows [0, rows_in[b]) of inlier[b] and [0, rows_nb[b]) of neighbor[b] are evaluated.  The caller
 * guarantees that every later row is a copy of one of those (the reference pads small sets by duplication,
 * test_region_grow.py:240,:252), so their logits equal the source row's bit for bit and the max-pool (:122-123) is
 * unchanged; logits of rows that are not evaluated are left unwritten.  A count of 0 skips the instance.
 * Needs LRG_FWD_FUSED (whole 32-row tiles of copies are skipped). */
int lrg_forward_rows(const LrgWeights *w, const float *inlier, const float *neighbor, int B, int n_inlier,
                     int n_neighbor, const int32_t *rows_in, const int32_t *rows_nb, float *add_logits,
                     float *rmv_logits, void *workspace, size_t workspace_bytes, unsigned flags, void *stream);

/* Workspace introspection for layer-by-layer parity tests: float offset / element count of a named
 * intermediate inside `workspace`.  kind: 0 conv[i] (inlier), 1 neighbor_conv[i], 2 pooled [B,2*C_last],
 * 3 add head hidden[i], 4 remove head hidden[i], 5 scratch (64 floats, reserved), 6 tile lists (int32: [0] inlier tile
 * count, [1] neighbour tile count, then B*ceil(n_inlier/32) inlier entries and B*ceil(n_neighbor/32) neighbour entries,
 * entry = instance * 64 + tile).
 * Returns 0, or LRG_EINVAL. */
int lrg_forward_workspace_view(const LrgWeights *w, int B, int n_inlier, int n_neighbor, int kind, int index,
                               size_t *offset_floats, size_t *count_floats);

/* One per-point layer  y = act(x @ w + bias)   (tf.nn.conv1d k=1 + bias_add + relu, :109-111).
 * x [rows,cin] (row stride ldx), w [cin,cout] (row stride ldw), y [rows,cout].
 * bias is [cout], or -- when rows_per_instance > 0 and bias_instance_stride > 0 -- one bias row per
 * instance: bias[(row / rows_per_instance) * bias_instance_stride + col] (the hoisted pooled-feature
 * product of the heads, :128-141).  pool_out (nullable, needs relu) receives
 * max over each instance's rows: pool_out[(row / rows_per_instance) * pool_stride + col]; it must be
 * zero-filled by the caller beforehand. */
int lrg_pointwise_layer(const float *x, int ldx, const float *w, int ldw, const float *bias, float *y, long rows,
                        int cin, int cout, int relu, int rows_per_instance, int bias_instance_stride,
                        float *pool_out, int pool_stride, void *stream);

/* Column max over each instance's rows: out[b*out_stride + c] = max_r x[b,r,c]   (tf.reduce_max axis=1, :122-123) */
int lrg_segmax(const float *x, float *out, int B, int rows, int C, int out_stride, void *stream);

/* Hoisted pooled-feature product of a head's first layer:
 * hb[b, c] = bias[c] + sum_k pooled[b,k] * w[k,c],  k < P   (the tiled part of the concat at :128-135) */
int lrg_head_pool_gemv(const float *pooled, const float *w, int ldw, const float *bias, float *hb, int B, int P,
                       int C, void *stream);

/* Final head layer, no ReLU: logits[r, 0..1] = h[r,:] @ w[C,2] + bias[2]   (:145-149, :158-162) */
int lrg_head_final(const float *h, const float *w, const float *bias, float *logits, long rows, int C, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Region-grow loop state (replaces the module-level state of test_region_grow.py:175-205)
 * ---------------------------------------------------------------------------------------------- */
enum {
    LRG_IDLE = 0,            /* slot not bound to work                                                     */
    LRG_ACTIVE = 1,          /* region growing                                                             */
    LRG_STOP_NONEIGHBOR = 2, /* test_region_grow.py:233-235                                                */
    LRG_STOP_NOEXPAND = 3,   /* :304-306                                                                   */
    LRG_STOP_STUCK = 4,      /* :294-297                                                                   */
    LRG_STOP_EMPTY = 5,      /* mask became empty; the reference raises at :292 -- defined as a stop here  */
    LRG_STOP_MAXSTEPS = 6,   /* optional safety cap (off when max_region_steps <= 0)                        */
    LRG_DONE = 7,            /* the slot's room has no unvisited seed left                                  */
    LRG_WAIT = 8,            /* finished its restarts, waiting for its group; also the state a host binds a
                                fresh group in (with seed = -1) so that lrg_advance picks the first seed    */
    LRG_PENDING = 9          /* lrg_grow_async with LrgAsyncBuffers.speculate > 1: the slot's region has stopped growing
                                (last_reason says why) and waits for the regions of the room's earlier seeds to be
                                committed first (test_region_grow.py:186-188 visits the seeds one after the other)    */
};

#define LRG_LOG_WORDS 8
/* One room, device-resident.  Arrays are per equalised point (n of them). */
typedef struct LrgRoom {
    const float *points;     /* [n,F] features as stacked at test_region_grow.py:165-172                    */
    const int32_t *voxels;   /* [n,3] rint(xyz/resolution)  (:175)                                          */
    const int32_t *obj_id;   /* [n] ground-truth instance id (:116), only for the GT flags (:230-231)        */
    const int32_t *order;    /* [n] seed order = argsort(curvatures) (:183)                                  */
    uint8_t *visited;        /* [n] (:178)                                                                  */
    int32_t *label;          /* [n] cluster_label before fill-in (:176)                                      */
    const uint64_t *hash_keys; /* voxel hash table (open addressing), hash_mask+1 entries                    */
    const int32_t *hash_vals;
    int32_t *region_log;     /* [n,LRG_LOG_WORDS] per committed seed: seed, steps, points, reason, labeled, restart, and the
                                number of sample slots whose argmax matched input_add / input_remove at the region's last
                                evaluated step (add_acc, remove_acc of learn_region_grow_util.py:175,180 times 512; -1: none) */
    int32_t n;
    int32_t hash_mask;
    int32_t next_cluster_id; /* (:177)                                                                      */
    int32_t seed_cursor;     /* position in `order` of the next candidate seed (:186-188)                    */
    int32_t n_regions;
    int32_t done;
    int32_t room_id;         /* RNG stream key and log tag                                                   */
    int32_t pad;
    const uint32_t *pvox;    /* nullable: [n] voxels relative to vox_origin packed x | y << 11 | z << 22 (lrg_voxel_pack); the
                                arrays visited / pvox must then start 16-byte aligned (word-wide loads of 4 points)   */
    int32_t vox_origin[3];   /* per-axis minimum voxel of the room                                           */
    int32_t chan_stride;     /* floats between two channels of chan_major                                    */
    const float *chan_major; /* nullable: the centred channels 0, 1, 6 .. F-1 (:243-247) channel-major,
                                chan_major[y * chan_stride + i] == points[i * F + (y < 2 ? y : y + 4)]: a region's points are
                                mostly runs of consecutive indices, so the median's keys (:241) come from a few dense lines
                                instead of one 4-byte word out of every F-float row                          */
    const int32_t *vgrid;    /* nullable (needs pvox / vox_origin): dense voxel grid of the room, x fastest,
                                vgrid[((vz - oz) * vgrid_dim[1] + (vy - oy)) * vgrid_dim[0] + (vx - ox)] = index of the point in
                                that voxel or -1 (lrg_voxel_grid_build).  The box query of a region (:221-229) then reads the cells
                                of its dilated box -- rows of consecutive ints -- instead of every point of the room, and a voxel
                                lookup (:273-287) is one load instead of a probe chain: 4 bytes per voxel of the room's bounding
                                box, a few MB per room out of 288 GB                                          */
    int32_t vgrid_dim[3];    /* voxels per axis of the room's bounding box                                   */
    int32_t pad2;
} LrgRoom;

/* One growing region instance.  A *group* of `group_size` consecutive slots shares one room and one seed
 * (random restarts, test_random_restart.py:169-197); greedy growing is group_size = 1, restarts = 1. */
typedef struct LrgSlot {
    uint8_t *cur;            /* [cap] currentMask (:197)                                                    */
    uint8_t *best;           /* [cap] best restart mask so far (restart :175-177); unused when restarts==1   */
    int32_t *cur_idx;        /* [cap] compacted indices of current points, index order (:221)                */
    int32_t *cand_idx;       /* [cap] compacted indices of expand candidates (:229)                          */
    int32_t room;            /* index into rooms[], -1 = none                                                */
    int32_t status;
    int32_t seed;            /* seed point (:186)                                                            */
    int32_t restart;         /* restart ordinal of the grow in progress                                      */
    int32_t step;            /* steps of the grow in progress (RNG counter)                                  */
    int32_t steps_total;     /* `steps` of the reference: never reset between restarts of a seed             */
    int32_t stuck;           /* (:204)                                                                       */
    int32_t nc;              /* len(currentPoints)                                                           */
    int32_t ne;              /* len(expandPoints)                                                            */
    int32_t updated;         /* (:278)                                                                       */
    int32_t count;           /* sum(currentMask) after the last update                                       */
    int32_t best_count;      /* restart_score of `best` (--scoring np), -1 = none                            */
    int32_t best_restart;
    int32_t last_reason;
    int32_t mn[3], mx[3];    /* minDims / maxDims (:199-200)                                                 */
    int32_t seq_mn[3], seq_mx[3]; /* seqMinDims / seqMaxDims (:201-202)                                      */
    int32_t target;          /* obj_id[seed] (:190)                                                          */
    int32_t pad;             /* 1 while cur_idx / cand_idx describe the current mask and bbox (set by lrg_box_query)  */
    int32_t *chunk_cnt;      /* [2 * ceil(cap / LRG_SCAN_CHUNK)] per-chunk (current, candidate) counts of lrg_box_query */
    int32_t scan_cnt;        /* lrg_bbox_stop scratch: members / min / max voxel of the updated mask, consumed (and    */
    int32_t scan_mn[3];      /*   reset) by lrg_advance                                                               */
    int32_t scan_mx[3];
    int32_t query;           /* lrg_box_query scratch: 1 if this call re-derives the slot's lists                     */
    int32_t acc_add;         /* sample slots whose argmax(add logits) == input_add at the last evaluated step (:175), -1 none */
    int32_t acc_rmv;         /* likewise for the remove head (:180)                                                     */
    double ml_score;         /* --scoring ml: log-likelihood of the masks sampled in the restart in progress (restart :251-271) */
    double ml_best;          /* ... of the banked restart                                                                */
    int32_t spec_pos;        /* speculation (ABI 9): position of the slot's seed in the room's seed order, INT32_MAX = no region in progress */
    int32_t spec_flags;      /* bit 0: the region in progress is void -- a region committed before it took a point inside a box it
                                had queried (:222-228 would have seen that point as visited); it is dropped and grown again         */
} LrgSlot;

#define LRG_SCAN_CHUNK 4096  /* points per workgroup of the chunked mask scans */

typedef struct LrgGrowParams {
    float resolution;        /* 0.1 (test_region_grow.py:27)                                                 */
    int32_t feature_size;
    int32_t n_inlier;        /* NUM_INLIER_POINT   (:22)                                                     */
    int32_t n_neighbor;      /* NUM_NEIGHBOR_POINT (:23)                                                     */
    int32_t cluster_threshold; /* 10 (:30)                                                                   */
    int32_t restarts;        /* NUM_RESTARTS; 1 = greedy                                                     */
    int32_t group_size;      /* slots per group; restarts are dealt round-robin over the group's slots       */
    int32_t max_region_steps;/* <= 0: no cap                                                                 */
    uint32_t rng_seed;       /* counter-stream key word 0 (key word 1 = room_id)                             */
    int32_t policy;          /* 0 net (:266-267), 1 threshold (:264-265), 2 ground truth (:268-269)          */
    int32_t scoring;         /* restart score (test_random_restart.py:171-174): 0 = 'np' points of the mask, 1 = 'ml' summed
                                log-likelihood of the sampled add / remove masks, one scalar per restart (upstream resets the
                                accumulator to a list at :194-196, which breaks it from the second restart on; implemented as
                                evidently intended).  For restarts 'ml' is computed by lrg_grow_step_packed only.  The beam search
                                (lrg_beam_level) reads the same switch for the score of its queue: see LrgBeamGroup.       */
} LrgGrowParams;

/* Bind the slots [first_slot, first_slot + group_size) to room `room` (-1: leave them idle), on the device: every slot
 * waits with seed -1, so the next advance picks the room's first seed (:186-188).  reset_room != 0 first returns the room to
 * its pristine state (visited / labels cleared, cursor at 0, :176-178); clear_masks != 0 clears the slots' masks over the
 * room they are leaving.  One launch, no host-to-device copy: safe to issue while other streams keep the host busy. */
int lrg_bind_group(LrgSlot *slots, LrgRoom *rooms, int first_slot, int group_size, int room, int reset_room, int clear_masks,
                   void *stream);

/* voxels[i,0..2] = rint(points[i,0..2] / resolution)   (test_region_grow.py:175) */
int lrg_voxelize(const float *points, int n, int F, float resolution, int32_t *voxels, void *stream);

/* pvox[i] = (vx - ox) | (vy - oy) << 11 | (vz - oz) << 22 for the room's voxels: one word per point for the box query and the
 * bounding-box passes of lrg_grow_step_packed.  (ox, oy, oz) = the per-axis minimum voxel; the room must span at most
 * 2048 x 2048 x 1024 voxels (the caller checks; out-of-range coordinates are clamped and set *overflow_flag, device int). */
int lrg_voxel_pack(const int32_t *voxels, int n, int ox, int oy, int oz, uint32_t *pvox, int32_t *overflow_flag, void *stream);

/* Dense voxel grid of a room (LrgRoom.vgrid): grid[gx * gy * gz] (x fastest) is filled with -1 and receives the index of the
 * point of each occupied voxel; (ox, oy, oz) = the per-axis minimum voxel, (gx, gy, gz) = the extent of the bounding box. */
int lrg_voxel_grid_build(const int32_t *voxels, int n, int ox, int oy, int oz, int gx, int gy, int gz, int32_t *grid, void *stream);

/* Build the room's voxel -> point-index table (replaces the tuple sets of :273,:277,:283-286).
 * keys must hold hash_mask+1 entries; *dup_flag (device int, zeroed by the caller) is set when two points
 * share a voxel (the path assumes an equalised room, :125-134). */
int lrg_voxel_hash_build(const int32_t *voxels, int n, uint64_t *keys, int32_t *vals, int hash_mask,
                         int32_t *dup_flag, void *stream);

/* Scan of the updated mask (:292-293): member count and min / max voxel of every ACTIVE slot that has taken a mask
 * update (slot.updated >= 0), reduced into slot.scan_*.  The stop / stuck decision of :291-306 is taken from those
 * values at the start of the following lrg_advance.  max_points = capacity of the per-slot masks (grid sizing). */
int lrg_bbox_stop(LrgSlot *slots, const LrgRoom *rooms, int n_slots, int max_points, const LrgGrowParams *params,
                  void *stream);

/* Commit finished seeds (:210-217 / restart :169-197), pick the next unvisited seed (:186-188) and reset
 * the group's slots (:197-204).  stats (device, LRG_STATS_WORDS x int64, nullable): see LrgStepBuffers. */
int lrg_advance(LrgSlot *slots, LrgRoom *rooms, int n_slots, const LrgGrowParams *params, int64_t *stats,
                void *stream);

/* Dilated voxel-box neighbour query + ordered compaction (:221-235): fills cur_idx/nc, cand_idx/ne; a slot
 * with ne == 0 stops with LRG_STOP_NONEIGHBOR. */
int lrg_box_query(LrgSlot *slots, const LrgRoom *rooms, int n_slots, int max_points, const LrgGrowParams *params,
                  void *stream);

/* center[s, c] = median over the slot's current points of channel c for c in {0,1} U [6,F), 0 elsewhere
 * (numpy.median, :241; only those channels are used, :243-247).  center is [n_slots,16]. */
int lrg_median(const LrgSlot *slots, const LrgRoom *rooms, int n_slots, const LrgGrowParams *params, float *center,
               void *stream);

/* Counter-stream subset sampling (:237-240, :249-252): positions into cur_idx / cand_idx,
 * sample_in [n_slots,n_inlier], sample_nb [n_slots,n_neighbor]. */
int lrg_sample(const LrgSlot *slots, const LrgRoom *rooms, int n_slots, const LrgGrowParams *params,
               int32_t *sample_in, int32_t *sample_nb, void *stream);

/* Gather + centre (:242-254): inlier [n_slots,n_inlier,F], neighbor [n_slots,n_neighbor,F];
 * gt_remove / gt_add (nullable) receive input_remove / input_add (:248,:254).
 * rows_in / rows_nb (nullable, [n_slots]) receive the number of distinct leading rows of each stacked set:
 * min(nc, n_inlier) / min(ne, n_neighbor) for an active slot (the rest are duplicates, :240,:252), 0 otherwise. */
int lrg_gather_center(const LrgSlot *slots, const LrgRoom *rooms, int n_slots, const LrgGrowParams *params,
                      const int32_t *sample_in, const int32_t *sample_nb, const float *center, float *inlier,
                      float *neighbor, int32_t *gt_remove, int32_t *gt_add, int32_t *rows_in, int32_t *rows_nb,
                      void *stream);

/* lrg_median + lrg_sample + lrg_gather_center in one pass per slot (counter stream): the preparation of a step,
 * test_region_grow.py:237-254.  Same outputs as the three calls. */
int lrg_prepare(const LrgSlot *slots, const LrgRoom *rooms, int n_slots, const LrgGrowParams *params, float *center,
                int32_t *sample_in, int32_t *sample_nb, float *inlier, float *neighbor, int32_t *gt_remove, int32_t *gt_add,
                int32_t *rows_in, int32_t *rows_nb, int32_t *tile_total, void *stream);
/* tile_total (nullable, device int32 block = workspace view kind 6 of an n_slots-instance forward): receives the lists of
 * live 32-row tiles for lrg_forward_rows(LRG_FWD_TILE_LISTS). */

/* Confidence + Bernoulli masks + voxel-set mask update (:262-288).
 * add_mask / rmv_mask (nullable, uint8 [n_slots,n]) : host-decided masks (reference-order RNG);
 * when NULL the masks are drawn on the device from the counter stream against
 * softmax(logits)[:,1].  Sets slot.updated, increments slot.step / steps_total and, when stats is
 * non-NULL, stats[2] (instance-steps taken).
 * sample_in / sample_nb (nullable): when given, logits were produced by lrg_forward_rows, i.e. only for the distinct
 * leading rows; slot j of a set with fewer points than slots then reads the logits of row sample[j] (its source). */
int lrg_mask_update(LrgSlot *slots, const LrgRoom *rooms, int n_slots, const LrgGrowParams *params,
                    const float *inlier, const float *neighbor, const float *center, const float *add_logits,
                    const float *rmv_logits, const int32_t *gt_remove, const int32_t *gt_add,
                    const uint8_t *add_mask, const uint8_t *rmv_mask, const int32_t *sample_in,
                    const int32_t *sample_nb, int64_t *stats, void *stream);

/* Device buffers of one lock-step iteration over n_slots slots (all caller-owned). */
typedef struct LrgStepBuffers {
    float *center;        /* [n_slots,16]                 */
    int32_t *sample_in;   /* [n_slots,n_inlier]           */
    int32_t *sample_nb;   /* [n_slots,n_neighbor]         */
    float *inlier;        /* [n_slots,n_inlier,F]         */
    float *neighbor;      /* [n_slots,n_neighbor,F]       */
    int32_t *gt_remove;   /* [n_slots,n_inlier]           */
    int32_t *gt_add;      /* [n_slots,n_neighbor]         */
    float *add_logits;    /* [n_slots,n_neighbor,2]       */
    float *rmv_logits;    /* [n_slots,n_inlier,2]         */
    void *workspace;      /* lrg_forward scratch          */
    size_t workspace_bytes;
    int64_t *stats;       /* LRG_STATS_WORDS x int64      */
    int32_t *rows_in;     /* [n_slots] rows to evaluate per slot (nullable pair: NULL = evaluate all 512+512 rows) */
    int32_t *rows_nb;
} LrgStepBuffers;

/* stats layout: [0] committed seeds, [1] rooms finished, [2] instance-steps taken, [3] hand-overs given up by lrg_grow_async (0 unless something is broken),
 * [4 + k % LRG_DONE_RING] = first slot of the k-th finished group (ring written by lrg_advance; the greedy front kernels add the
 * room index: slot | room << 32). */
#define LRG_DONE_RING 1020
#define LRG_STATS_WORDS (4 + LRG_DONE_RING)

/* One whole lock-step iteration with device-side (counter-stream) randomness -- the body of the
 * `while True` loop at test_region_grow.py:208-306 for every slot at once:
 *   lrg_bbox_stop; advance_rounds x (lrg_advance; lrg_box_query); lrg_prepare (= lrg_median + lrg_sample +
 *   lrg_gather_center); lrg_forward_rows; lrg_mask_update.
 * `weights` and `buffers` are HOST structs of device pointers. */
int lrg_grow_step(LrgSlot *slots, LrgRoom *rooms, int n_slots, int max_points, const LrgGrowParams *params,
                  const LrgWeights *weights, const LrgStepBuffers *buffers, int advance_rounds, unsigned forward_flags,
                  void *stream);

/* ------------------------------------------------------------------------------------------------
 * Packed-row formulation of the same iteration (the default of the batched loop).
 *
 * A stacked set with fewer points than sample slots is padded by re-drawing its own rows (test_region_grow.py:240,:252);
 * LrgNet is row-wise up to the max-pool, which ignores duplicates.  Here only the DISTINCT rows of every slot are
 * gathered, back to back for all slots (one packed array per branch), and the network runs on dense 32-row tiles of
 * those arrays: a tile may hold rows of several slots; the max-pool (:122-123) and the hoisted per-instance bias
 * (:128-141) are applied per run of rows of one slot.  Logits come back per packed row; sample slot j of a padded set
 * reads the logits of its source row.  Results are bit-identical to lrg_grow_step.
 * ---------------------------------------------------------------------------------------------- */

/* LrgNet on packed rows.  x_in / x_nb [row_cap,F] hold nrows[0] / nrows[1] valid rows (device int32 pair);
 * center (nullable, [n_inst,16]): when given, the rows are stored UNCENTRED and row r enters the network as
 * x[r,c] - center[row_inst[r]*16 + c] (test_region_grow.py:243-247 applied while the rows are staged; center is 0 on the
 * channels the reference leaves alone);
 * row_inst_in / row_inst_nb [row_cap] name the instance (0 <= . < n_inst) of each row, rows of one instance being
 * contiguous; row_cap is a multiple of LRG_ROW_TILE.  add_logits [row_cap,2] (per neighbour row, net.add_output :149),
 * rmv_logits [row_cap,2] (per inlier row, net.remove_output :162).
 * nrows_heads (nullable, device int32 pair): when given, the row counts are handed over to it and nrows is zeroed
 * between the branch and the head kernels, so that the caller's next allocation pass starts from zero.
 * flags: LRG_FWD_POOL_ZEROED = the pooled block of the workspace (lrg_forward_packed_pooled_view) is zero on entry.
 * Needs the layer widths the fused kernels are built for (lite 0/1/2). */
size_t lrg_forward_packed_workspace_bytes(const LrgWeights *w, int n_inst, int row_cap);
int lrg_forward_packed_pooled_view(const LrgWeights *w, int n_inst, int row_cap, size_t *offset_floats, size_t *count_floats);
int lrg_forward_packed(const LrgWeights *w, const float *x_in, const float *x_nb, const float *center, const int32_t *row_inst_in,
                       const int32_t *row_inst_nb, int32_t *nrows, int32_t *nrows_heads, int n_inst, int row_cap,
                       float *add_logits, float *rmv_logits, void *workspace, size_t workspace_bytes, unsigned flags,
                       void *stream);

/* Device buffers of one packed iteration over n_slots slots (all caller-owned; counters zero before the first call). */
typedef struct LrgPackedBuffers {
    float *center;          /* [n_slots,16]                                                                  */
    int32_t *sample_in;     /* [n_slots,n_inlier]   sample positions (:237-240); written by lrg_front_kernel only: the greedy */
    int32_t *sample_nb;     /* [n_slots,n_neighbor] (:249-252)   front kernels draw them again in their mask update          */
    float *x_in;            /* [row_cap,F] packed distinct inlier rows of all slots (:245-247)               */
    float *x_nb;            /* [row_cap,F] packed distinct neighbour rows (:243-244,:253)                    */
    int32_t *row_slot_in;   /* [row_cap] slot of each packed row                                             */
    int32_t *row_slot_nb;
    float *upd_in;          /* [n_slots,n_inlier,4]   per slot, for its distinct inlier rows j: columns 0..2 of the packed row and
                                input_remove of its point (:248) as 0.0 / 1.0 -- what the NEXT mask update (:262-288) needs of
                                the row, in storage of the slot's own (16-byte aligned).  The packed arrays are allocated from row 0
                                again by every launch: a slot whose workgroup starts late must not look for last iteration's rows there */
    float *upd_nb;          /* [n_slots,n_neighbor,4] the same for the neighbour rows and input_add (:254)    */
    float *rmv_logits;      /* [row_cap,2] per packed inlier row                                             */
    float *add_logits;      /* [row_cap,2] per packed neighbour row                                          */
    int32_t *slot_rows;     /* [n_slots,4] rows_in, rows_nb, first packed inlier row, first packed neighbour row */
    int32_t *counters;      /* [4] packed rows allocated (in, nb) and their hand-over copy for the heads      */
    void *workspace;        /* lrg_forward_packed_workspace_bytes(w, n_slots, row_cap), 256-byte aligned       */
    size_t workspace_bytes;
    int64_t *stats;         /* LRG_STATS_WORDS x int64, as LrgStepBuffers                                      */
    int32_t row_cap;        /* multiple of LRG_ROW_TILE, >= n_slots * max(n_inlier, n_neighbor) rounded up to 16: a slot's
                                rows are allocated in multiples of 8, the padding being copies of its last row    */
    int32_t rooms_have_pvox; /* 1: every room carries pvox (and 16-byte aligned visited / pvox): enables the single-launch greedy
                                front kernel with word-wide room scans                                          */
    int32_t *slot_big;      /* nullable with rooms_have_pvox = 0: [n_slots,2] zero-filled ONCE and owned by these buffers for good:
                                (rows prepared this iteration, running tag of the slot's centres) -- the medians come from a
                                second, (slot, channel)-parallel launch                                            */
    int64_t *phase_ticks;   /* nullable: [n_slots,2] accumulators of wall_clock64() ticks the slot's workgroup spent in (0) mask
                                update / stop decision / commit -- the reference's 'inlier' bucket, test_region_grow.py:260-306 --
                                and (1) box query / median / sampling / gather -- its 'neighbor' bucket, :219-254            */
} LrgPackedBuffers;

/* One lock-step iteration, packed rows: lrg_front_kernel (mask update of the previous evaluation :262-288, stop decision
 * :291-306, commit / next seed :186-217, box query :221-235, medians :241, sampling :237-252, gather :242-254) and
 * lrg_forward_packed -- five launches (front, medians, branch stacks, pooled GEMM, head stacks; six with restart groups: update,
 * group commit, query + medians + gather, then the three of the network).
 * Slot masks (LrgSlot.cur) must be 4-byte aligned;
 * rooms of up to 131072 points, n_inlier / n_neighbor <= 1024; larger: lrg_grow_step. */
int lrg_grow_step_packed(LrgSlot *slots, LrgRoom *rooms, int n_slots, int max_points, const LrgGrowParams *params,
                         const LrgWeights *weights, const LrgPackedBuffers *buffers, void *stream);
/* The two halves of lrg_grow_step_packed as separate calls (so that a caller can put events between them):
 * lrg_front_step = everything up to the packed rows; then lrg_forward_packed(weights, x_in, x_nb, centre, row_slot_in,
 * row_slot_nb, counters, counters + 2, n_slots, row_cap, add_logits, rmv_logits, workspace, workspace_bytes,
 * LRG_FWD_POOL_ZEROED, stream) with centre = lrg_packed_rows_center(params, buffers): the buffers' centre array when the front
 * kernels store uncentred rows (greedy growing on rooms with packed voxel words), NULL when they store centred rows. */
int lrg_front_step(LrgSlot *slots, LrgRoom *rooms, int n_slots, int max_points, const LrgGrowParams *params,
                   const LrgWeights *weights, const LrgPackedBuffers *buffers, void *stream);
const float *lrg_packed_rows_center(const LrgGrowParams *params, const LrgPackedBuffers *buffers);

/* `iterations` calls of lrg_grow_step_packed captured into a HIP graph on `stream` (not the null stream; weights->packed
 * set).  Nothing runs at creation.  lrg_step_graph_launch replays them with one host call. */
int lrg_step_graph_create(LrgSlot *slots, LrgRoom *rooms, int n_slots, int max_points, const LrgGrowParams *params,
                          const LrgWeights *weights, const LrgPackedBuffers *buffers, int iterations, void *stream,
                          void **graph_out);
int lrg_step_graph_launch(void *graph, void *stream);
int lrg_step_graph_destroy(void *graph);

/* ------------------------------------------------------------------------------------------------
 * Free-running iterations: the same loop (test_region_grow.py:208-306), every slot at its own pace inside ONE launch.
 * lrg_grow_step_packed is five launches over all slots, each as long as its slowest slot or tile; rooms are independent
 * (:110-183), so here a slot's stages -- front (mask update :262-288, stop decision :291-306, commit / next seed :186-217, box
 * query :221-235, medians :241, sampling :237-252, gather :242-254), branch stacks, pooled product, head stacks
 * (learn_region_grow_util.py:106-162) -- are ordered by that slot's own arrival counters: front workgroups serve the slots,
 * the other CUs run tile tasks from a queue (csrc/lrg_async.inl).  Greedy growing (restarts = group_size = 1) on rooms with
 * packed voxel words, n_inlier / n_neighbor <= 512, lite 0 / 2 -- LRG_EINVAL otherwise (use lrg_grow_step_packed).
 * State between calls is exactly that of lrg_grow_step_packed (a call ends every slot between two evaluations, logits in
 * place), so the two may alternate on the same buffers; results are identical bit for bit.
 * ---------------------------------------------------------------------------------------------- */
#define LRG_REG_TILE_AUTO_MIN 1    /* register-tile launches (branch_waves = 1) by default from this many (up to 24 slots a branch tile is two tasks: one room +14 %, x 3 regions +7 %, 16 rooms +3 %) ... */
#define LRG_REG_TILE_AUTO_MAX 176  /* ... to this many slots in flight: 16 (x 3 regions) / 34 / 68 / 100 / 136 / 160 slots +6 / +11.5 / +9.6 / +9.1 / +4 / +4.6 % over the one-kernel launch,
                                      192: -1.7 % (two teams per CU are too few there), eight 100 k-point scenes x 3 regions: -0.7 % (profiles/r06_reg_tiles_slots.txt) */
typedef struct LrgAsyncBuffers {
    int32_t *queue;             /* lrg_grow_async_queue_bytes(n_slots) bytes, 256-byte aligned: task ring + control words (cleared by every call) */
    size_t queue_bytes;
    int32_t *sync;              /* [n_slots, 16] arrival counters of the slots (cleared by every call)                     */
    int32_t front_workgroups;   /* workgroups serving the slots (each up to 8 of them), 0 = default                       */
    int32_t teams;              /* tile teams (four wavefronts) per worker workgroup: 1 .. 4 (4: two of them run branch tiles only), 0 = default */
    int32_t compute_units;      /* workgroups of the launch in all (front + worker), at most one per CU of the device; 0 = all CUs */
    int32_t poll_sleep;         /* idle tile teams poll the queue every poll_sleep x ~0.25 us; 0 = default                  */
    int32_t branch_parts;       /* tasks per branch tile (1, 2 or 4: they share the four column blocks of its pooled layer and each run the
                                   layers before it again); 0 = by the number of slots (2 up to 12 slots, else 1)                    */
    int32_t gemv_units;         /* 0 = default: up to 176 slots the heads' pooled kernels stay in the LDS of 2 C / 32 workgroups of their own (32
                                   columns each; a slot's pooled product = one 4 KB row in, 32 sums out per unit, and its head tiles start
                                   beside it) where that fits; 1 = also above 176 slots; -1 = the tile teams compute it in 128-column
                                   blocks from L2                                                                                 */
    int32_t *room_queue;        /* nullable: rooms waiting for a slot -- [0] rooms handed out so far (the caller zeroes it when it refills
                                   the queue), [1] rooms queued, [2 + k] = room index | reset << 30 (reset: clear visited / labels /
                                   cursor first, as lrg_bind_group does).  A slot whose room is finished (or that has none) takes the
                                   next one inside the launch; finished rooms appear in the stats ring as slot | room << 32      */
    uint64_t *work;             /* nullable: [8] running totals (never cleared by the library) of what the launches evaluated: LrgNet
                                   evaluations, distinct inlier rows, distinct neighbour rows, 32-row tiles per stack (branch = head) --
                                   the algorithmic FLOPs of the launches follow from these; [4] regions voided and grown again under
                                   `speculate`, [5] the evaluations those regions had taken, [6] of these: steps counted in stats[2]
                                   (ABI 9: 8 words, was 4)                                                                          */
    /* In-launch fill-in (ABI 8; all five non-NULL, 13 features): a room that finishes during the launch gets its 1-NN fill-in
       (test_region_grow.py:308-316) from tile teams of the same launch instead of from lrg_nn1_fill_batch between launches; such rooms
       carry bit 31 in the slot word of their done-ring entry.  The arenas are laid out like the label arena the rooms' LrgRoom.label
       pointers point into (fill_label_base = its first element): a room's lists live at its label offset.                              */
    int32_t *fill_list;         /* [points of all rooms] int32                                                                          */
    uint64_t *fill_best;        /* [points of all rooms] 8-byte aligned                                                                  */
    int32_t *fill_sync;         /* [fill_rooms, 4] int32                                                                                 */
    const int32_t *fill_label_base;
    int32_t *fill_out_base;     /* the filled labels (label_out of lrg_nn1_fill), same layout                                            */
    int32_t fill_rooms;         /* rooms in the LrgRoom array                                                                            */
    int32_t fill_wgs;           /* worker workgroups with a team for the fill-in ring (one more than the others have, up to three tile teams;
                                   else their last team); 0 = default (64)                                                                */
    int32_t rows16;             /* 1: buffers->x_in / x_nb hold row_cap x 16 floats (16-byte aligned): lrg_grow_async gathers its rows at a 64-byte stride
                                   in 16-byte pieces (9 .. 16 features); 0: row_cap x feature_size floats, one element per store (ABI 8)            */
    int32_t speculate;          /* K > 1 (ABI 9): the slots are groups of K (slots g K .. g K + K - 1, one front workgroup per group), all bound to the SAME room:
                                   the regions of the room's next K unvisited seeds grow side by side and are committed in seed order; a region is dropped and
                                   grown again when a region committed before it contains a point inside any dilated box it has queried -- otherwise its
                                   queries saw exactly what the sequential loop (:186-188,:210-217,:227-228) would have shown them.  Same regions, same labels;
                                   for the few-rooms corner (one room or scene per GPU), where a room's chain of dependent steps leaves the chip idle.
                                   n_slots must be a multiple of K; the caller binds whole groups (lrg_bind_group with group_size K); 0 / 1 = off           */
    int32_t branch_waves;       /* (ABI 10; was `reserved2`) two-kernel launches: the CUs that run tiles as a SECOND kernel (512 threads, up to 256 VGPRs) resident beside the
                                   front workgroups' and units' kernel (csrc/lrg_wave_tile.inl; same results bit for bit in every form):
                                     1 = REGISTER TILES: a branch tile (learn_region_grow_util.py:106-123) by a team of four wavefronts that each run layers 0 - 2 in
                                         registers, meet once in LDS behind layer 3 and take a quarter of the pooled layer each; the other team of the CU runs head tiles;
                                     4 / 8 = one-wavefront tasks: a PREFIX task (layers 0 - 3) and four POOL tasks (a quarter of the pooled layer) per tile, on CUs that
                                         hold the kernels of their stage in LDS, that many wavefronts per such CU (measured slower at every slot count: kept as an option);
                                     0 = by the slot count: register tiles from LRG_REG_TILE_AUTO_MIN to LRG_REG_TILE_AUTO_MAX slots; -1 = one kernel, team tiles.
                                   Needs the paper's network (13 -> 64 -> 64 -> 64 -> 128 -> 512), rows16, no tail_ctl / pool_rows, all CUs of the device. */
    int32_t start_wait_us;      /* the launch's start rendezvous (all its workgroups must be running at once): how long the front workgroups wait for the
                                   others before the launch gives up with reason 6; 0 = default: the launch budget + 20 ms (a kernel of another stream that
                                   holds CUs for up to one budget is waited out, something that never leaves is reported)  (ABI 9; was `reserved`) */
    float *pool_rows;           /* nullable: lrg_grow_async_pool_rows_bytes(weights, n_slots) bytes, 16-byte aligned -- with the pooled-product units a
                                   branch tile leaves the column maxima of its rows as one row here (16-byte stores) and the units take the maximum
                                   over a slot's tiles; NULL: one atomicMax per column and tile on the pooled feature (ABI 8)              */
    size_t pool_rows_bytes;
    uint64_t *debug_ticks;      /* nullable: [64] accumulators (never cleared by the library) of wall-clock ticks by stage of the
                                   launch, for tools/free_run_perf.py (layout: csrc/lrg_async.inl, LrgAsyncArgs.dbg)            */
    /* Shared tail tiles (ABI 9; tail_ctl non-NULL, tail_rows > 0, rows16): a slot's rows beyond its last full 32-row tile (16 of ~91 rows per side on
       average: as padded tiles of the slot's own they were 18 % of all tile rows) go to `tail_rows` rows per side that ALL slots share -- rows
       [n_slots * row_stride, + tail_rows) of the row arrays (buffers->row_cap and the workspace must cover them and 32 rows more) -- so that the tails of several slots fill one
       branch tile.  Same results bit for bit (the shared tile is lrg_forward_packed's tile: runs of rows, per-run max-pool).  When a launch runs out of
       shared rows the slots pad tiles of their own again.                                                                                        */
    int32_t *tail_ctl;          /* lrg_grow_async_tail_bytes(n_slots, tail_rows) bytes, 64-byte aligned (cleared by every call)                    */
    int32_t tail_rows;          /* a multiple of 32                                                                                                */
    int32_t tail_close_us;      /* a slot closes its last shared tile (the rest of its rows stay empty) when nobody has filled it up that long after the
                                   slot's rows went out; 0 = default (2 us), -1 = at once                                                          */
} LrgAsyncBuffers;

size_t lrg_grow_async_queue_bytes(int n_slots);
size_t lrg_grow_async_tail_bytes(int n_slots, int tail_rows);
size_t lrg_grow_async_pool_rows_bytes(const LrgWeights *weights, int n_slots);

/* One free-running launch: every slot takes up to max_steps evaluations (grow steps), and starts no new one once budget_us
 * microseconds have passed since the launch began (0 = no time limit); slots whose room is finished or that are not bound
 * leave at once.  `buffers` are those of lrg_grow_step_packed with row_cap >= n_slots * 32 * ceil(max(n_inlier, n_neighbor) / 32)
 * (slot s owns that many rows from s * that number on).
 * Residency: the launch is one workgroup per CU whose roles wait for each other, so all of them must run at once.  Refused with
 * LRG_ERESIDENCY, before anything is enqueued, when the kernel does not fit a CU or the stream's CU mask (hipExtStreamCreateWithCUMask)
 * leaves it fewer CUs than the launch has workgroups (AsyncBuffers.compute_units: pass the number of CUs the stream may use).  CUs held
 * by somebody else (another process, a kernel of another stream) cannot be seen from the host: every workgroup reports in when it
 * starts, and a launch whose workgroups have not all started within 20 ms gives up at once (reason 6 in stats[3]) instead of
 * stalling.  A hand-over that was given up is counted in stats[3] (low word: workgroups that left this way, high word: sum of
 * their reasons -- 1 launch past its time limit, 2 a team waited too long for a task, 3 a team lost a wavefront at a barrier, 4 / 5 a
 * pooled-product unit / a head tile waited too long, 6 not all workgroups resident); the caller must treat a non-zero count as a
 * failed call. */
int lrg_grow_async(LrgSlot *slots, LrgRoom *rooms, int n_slots, int max_points, const LrgGrowParams *params,
                   const LrgWeights *weights, const LrgPackedBuffers *buffers, const LrgAsyncBuffers *async_buffers,
                   int max_steps, int budget_us, void *stream);

/* A stream whose kernels run only on the compute units set in `mask` (bit i of word i / 32; hipExtStreamCreateWithCUMask).
 * Meant for lanes (slot groups iterating independently on their own streams, the batched scheduler of north_star) on disjoint CU
 * sets.  mask = NULL: a plain non-blocking stream.
 * Measured on one MI355X: no gain at two lanes (lanes do not compete for CUs, profiles/r02_lanes_cu_partition_sweep.txt), and three
 * masked streams of a spin-kernel microbenchmark did not finish (tools/stream_overlap.hip) -- an option for experiments, off by default. */
int lrg_stream_create_cu_mask(const uint32_t *mask, int words, void **stream);
int lrg_stream_destroy(void *stream);

/* ------------------------------------------------------------------------------------------------
 * Beam search (test_beam_search.py:143-290) with the queue on the device.
 * A room in flight is a group of beam_width * search_width consecutive slots (child (qid, search id) = slot qid * search_width
 * + search id).  lrg_beam_level = one level of every room in flight: lrg_beam_advance (children of the last level -> next queue
 * by score, :275-287; stall test / commit of the head, :188-198,:289-293; next seed, :154-174; next children into the slots),
 * then the loop's kernels over all slots (box query, median, sampling, gather, LrgNet on the distinct rows, the 'ml' score where
 * asked for, mask update, scan of the updated masks).  No host decision in between; finished rooms appear in the stats ring
 * (first slot of the group).
 * The score (LrgGrowParams.scoring, test_beam_search.py:275-280) is the sort key of every level: 0 = 'np', the points of the child's
 * mask; 1 = 'ml', the parent's score plus the log-likelihood of the masks the child sampled (lrg_beam_ml_score, :237-257,:273),
 * carried from level to level in q_score / LrgSlot.ml_score.  The best beam_width children by that key (descending, ties in child
 * order) form the next queue, and emptied masks are dropped from it AFTERWARDS (csrc/lrg_beam_select.h).
 * ---------------------------------------------------------------------------------------------- */
/* One record of the optional trace: what lrg_beam_advance chose at one evaluated level of one seed. */
typedef struct LrgBeamTraceRec {
    int32_t room;            /* index into rooms[]                                                                       */
    int32_t seed;            /* seed point                                                                               */
    int32_t level;           /* level of the queue whose children were evaluated                                         */
    int32_t n;               /* entries below: the best beam_width children BEFORE the emptied masks are dropped         */
    int32_t ordinal[16];     /* child ordinal qid * search_width + search id                                             */
    int32_t size[16];        /* points of its mask; 0 = emptied, dropped from the queue                                  */
    double score[16];        /* its key: 'ml' the log-likelihood, 'np' the size as a double                              */
} LrgBeamTraceRec;
typedef struct LrgBeamGroup {
    uint8_t *parent;         /* [beam_width, cap] masks of the queue entries                                             */
    int32_t cap;             /* row stride of parent                                                                     */
    int32_t room;            /* index into rooms[], -1 = none (the host binds a group by writing room, seed = -1, pending = done = 0) */
    int32_t seed;            /* seed point in progress, -1 = pick the next                                               */
    int32_t level, stuck, steps, nq;
    int32_t pending;         /* 1: the slots hold the evaluated children of the current queue                            */
    int32_t done;            /* the room has no unvisited seed left                                                      */
    int32_t seq_mn[3], seq_mx[3];
    int32_t q_count[16], q_parent[16];       /* queue entries: mask size, parent buffer (-1 = the seed alone)            */
    int32_t q_mn[16][3], q_mx[16][3];        /* their bounding boxes                                                      */
    int32_t trace_cap;       /* records `trace` holds                                                                    */
    double q_score[16];      /* their 'ml' scores (0 for the seed-only head, :164; 0 under 'np')                          */
    LrgBeamTraceRec *trace;  /* nullable, device: one record per (group, evaluated level), written at index atomicAdd(trace_count, 1) --  */
    int32_t *trace_count;    /*   in level order within a room; records beyond trace_cap are counted, not written (all groups may share both) */
} LrgBeamGroup;
int lrg_beam_advance(LrgBeamGroup *groups, LrgSlot *slots, LrgRoom *rooms, int n_groups, int beam_width, int search_width,
                     const LrgGrowParams *params, int64_t *stats, void *stream);
int lrg_beam_level(LrgBeamGroup *groups, LrgSlot *slots, LrgRoom *rooms, int n_groups, int beam_width, int search_width, int max_points,
                   const LrgGrowParams *params, const LrgWeights *weights, const LrgStepBuffers *buffers, unsigned forward_flags,
                   void *stream);
/* The 'ml' score of one evaluated level alone (what lrg_beam_level runs between the network and the mask update when
 * params->scoring == 1): for every ACTIVE slot, slot.ml_score = (slot.ml_score + add side) + remove side, where a side is the sum over
 * ALL sample rows (padded copies included) of log(conf_i) / n_neighbor if the row's un-centred, re-voxelised point lies in a voxel
 * whose draw fired, else log(1 - conf_i) / n_neighbor -- both sides divide by n_neighbor (:255,:257).  float32 terms as NumPy computes
 * them, each side summed in float64 in a fixed order (no atomics: the same bits every run).  The draws are those lrg_mask_update takes
 * next (same keys, same policy switch; slot.step must still be the level's).  Reads buffers->center, inlier, neighbor, add_logits,
 * rmv_logits, gt_add / gt_remove (policy 2), and sample_in / sample_nb where rows_in and rows_nb are set (the network then ran on the
 * distinct leading rows only, and a padded row's logits are its source row's).  n_inlier, n_neighbor <= 1024.  Idle slots are left alone. */
int lrg_beam_ml_score(LrgSlot *slots, const LrgRoom *rooms, int n_slots, const LrgGrowParams *params, const LrgStepBuffers *buffers,
                      void *stream);

/* 1-NN fill-in of unlabeled points in all F feature dims, first-min ties (:308-316). */
int lrg_nn1_fill(const float *points, int n, int F, const int32_t *label_in, int32_t *label_out, void *stream);
/* The same result through a tiled search that reads the candidate rows once per 64 unlabeled points.  workspace: lrg_nn1_fill_workspace_bytes(n) bytes of device memory, 256-byte aligned.  F <= 13.  (A NaN distance
 * sorts after every number here; numpy.argmin would return the first NaN.) */
size_t lrg_nn1_fill_workspace_bytes(int n);
int lrg_nn1_fill_ws(const float *points, int n, int F, const int32_t *label_in, int32_t *label_out, void *workspace,
                    size_t workspace_bytes, void *stream);
/* Several rooms at once (the rooms that finish during one free-running launch): the same result as lrg_nn1_fill_ws room by room, three
 * launches per 64 rooms.  `jobs` is host memory; n = 0 rooms are skipped.  workspace: lrg_nn1_fill_batch_workspace_bytes(jobs, n_jobs) bytes. */
typedef struct LrgFillJob {
    const float *points;         /* [n, F] */
    const int32_t *label_in;     /* [n], 0 = unlabeled */
    int32_t *label_out;          /* [n] */
    int32_t n;
    int32_t reserved;
} LrgFillJob;
size_t lrg_nn1_fill_batch_workspace_bytes(const LrgFillJob *jobs, int n_jobs);
int lrg_nn1_fill_batch(const LrgFillJob *jobs, int n_jobs, int F, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * tf_ops/grouping replacements.  Same argument order as the reference launchers
 * (tf_ops/grouping/tf_grouping_g.cu:125-141) plus a trailing stream; extern "C"; int return.
 * ---------------------------------------------------------------------------------------------- */
/* queryBallPointLauncher (tf_grouping_g.cu:125; kernel :3-36).  Rows with no hit are zero-filled. */
int lrg_query_ball_point(int b, int n, int m, float radius, int nsample, const float *xyz1, const float *xyz2,
                         int *idx, int *pts_cnt, void *stream);
/* query_ball_point + group_point(xyz, idx) + group_point(points, idx) as the reference chains them in sample_and_group (train_pointnet.py:113-121), in ONE launch:
 * idx [b,m,nsample], pts_cnt [b,m] as lrg_query_ball_point; grouped_xyz [b,m,nsample,3] = xyz1 rows at idx (minus the query's coordinates when subtract_center: the
 * float32 subtraction of :117); grouped_points [b,m,nsample,c] = points rows at idx (points and grouped_points both NULL: skipped).  nsample <= 4096.  (ABI 9) */
int lrg_query_ball_group(int b, int n, int m, int c, float radius, int nsample, const float *xyz1, const float *xyz2, const float *points, int *idx,
                         int *pts_cnt, float *grouped_xyz, float *grouped_points, int subtract_center, void *stream);

/* selectionSortLauncher (tf_grouping_g.cu:129; kernel :83-123): full [b,m,n] outputs, first k sorted. */
int lrg_selection_sort(int b, int n, int m, int k, const float *dist, int *outi, float *out, void *stream);
/* groupPointLauncher (tf_grouping_g.cu:133; kernel :40-57) */
int lrg_group_point(int b, int n, int c, int m, int nsample, const float *points, const int *idx, float *out,
                    void *stream);
/* groupPointGradLauncher (tf_grouping_g.cu:137; kernel :61-78); grad_points must be zeroed by the caller
 * (the reference op does cudaMemset at tf_grouping.cpp:204). */
int lrg_group_point_grad(int b, int n, int c, int m, int nsample, const float *grad_out, const int *idx,
                         float *grad_points, void *stream);
/* knn_point (tf_grouping.py:48-73) in one kernel: val [b,m,k], idx [b,m,k] = the first k entries of selectionSortLauncher applied
 * to the distance matrix sum_c (xyz1[b,n,c]-xyz2[b,m,c])^2, bit for bit (same swap sequence, so the same order among equal
 * distances), without the b x m x n matrix ever existing.  n <= 4096 (a row lives in registers), k <= min(n, 512); LRG_EINVAL - 2 beyond. */
int lrg_knn_topk(int b, int n, int m, int c, int k, const float *xyz1, const float *xyz2, float *val, int *idx, void *stream);
/* dist[b,m,n] = sum_c (xyz1[b,n,c]-xyz2[b,m,c])^2 -- the matrix knn_point builds at tf_grouping.py:62-65 */
int lrg_pairwise_sqdist(int b, int n, int m, int c, const float *xyz1, const float *xyz2, float *dist, void *stream);

/* ------------------------------------------------------------------------------------------------
 * tf_ops/sampling and tf_ops/3d_interpolation replacements.  Argument order of the reference launchers
 * (tf_ops/sampling/tf_sampling_g.cu:194-212, tf_ops/3d_interpolation/tf_interpolate.cpp:60,107,131) plus a trailing stream;
 * extern "C"; int return.  No entry point allocates: workspaces come from the caller.
 * ---------------------------------------------------------------------------------------------- */
/* farthestpointsamplingLauncher (kernel tf_sampling_g.cu:105-170): inp [b,n,3] -> out [b,m] int32.  out[b,0] = 0; each step
 * picks the point of largest running minimum squared distance (fp32, no FMA, minima start at 1e38f).  Tie rule (the
 * reference's 512-thread stride scan with strict > and its left-keeping tree): among equal maxima the smallest
 * (k mod 512, k) wins; with m > n, once every minimum is 0, index 0 repeats.  n <= 16384 runs from registers and temp may be
 * NULL; larger n needs temp = b*n floats of device memory (LRG_EINVAL - 3 without it).  m <= 0 writes nothing. */
int lrg_farthest_point_sample(int b, int n, int m, const float *inp, float *temp, int *out, void *stream);
/* gatherpointLauncher (:172-181): out [b,m,3] = inp [b,n,3] rows at idx [b,m]; an index outside [0,n) gathers zeros. */
int lrg_gather_point(int b, int n, int m, const float *inp, const int *idx, float *out, void *stream);
/* scatteraddpointLauncher (:183-192): inp_g [b,n,3] += out_g [b,m,3] at idx, fp32 atomics; inp_g zeroed by the caller. */
int lrg_scatter_add_point(int b, int n, int m, const float *out_g, const int *idx, float *inp_g, void *stream);
/* probsampleLauncher (:198-201): temp [b,n] = inclusive cumsum of inp_p [b,n] (summation order: csrc/lrg_sampling.hip), then
 * out [b,m] = the smallest j with temp[j] >= inp_r[b,m] * temp[n-1] by the reference's binary search (:90-104). */
int lrg_prob_sample(int b, int n, int m, const float *inp_p, const float *inp_r, float *temp, int *out, void *stream);
/* threenn_cpu (tf_interpolate.cpp:60-104), bit for bit: xyz1 [b,n,3] unknown, xyz2 [b,m,3] known -> dist [b,n,3] squared
 * distances, idx [b,n,3]; the first index wins ties; with m < 3 the missing slots keep idx 0 and dist inf ((float)1e40). */
int lrg_three_nn(int b, int n, int m, const float *xyz1, const float *xyz2, float *dist, int *idx, void *stream);
/* threeinterpolate_cpu (:107-128), bit for bit: out [b,n,c] = (p[i1] w1 + p[i2] w2) + p[i3] w3, points [b,m,c], idx and
 * weight [b,n,3]; an index outside [0,m) contributes 0. */
int lrg_three_interpolate(int b, int m, int c, int n, const float *points, const int *idx, const float *weight, float *out, void *stream);
/* threeinterpolate_grad_cpu (:131-155): grad_points [b,m,c] += grad_out [b,n,c] * w at idx, fp32 atomics; grad_points zeroed
 * by the caller (as lrg_group_point_grad). */
int lrg_three_interpolate_grad(int b, int n, int c, int m, const float *grad_out, const int *idx, const float *weight,
                               float *grad_points, void *stream);
/* The interpolation that opens pointnet_fp_module (train_pointnet.py:145-150) in ONE launch: three_nn, then
 * inv_i = 1/max(d_i, 1e-10f) (correctly rounded), norm = (inv_0 + inv_1) + inv_2, w_i = inv_i / norm, then three_interpolate of
 * points [b,m,c] into out [b,n,c].  dist, idx, weight [b,n,3] are optional outputs (NULL: not written).  m >= 1. */
int lrg_three_nn_interpolate(int b, int n, int m, int c, const float *xyz1, const float *xyz2, const float *points, float *dist,
                             int *idx, float *weight, float *out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * benchmarks.py region-growing baselines (benchmarks.py:127-142 thresholds, :251-378 edges on the 26-neighbour voxel graph,
 * :380-416 components and numbering).  extern "C"; int return; no entry point allocates.  DESIGN.md §3.8.
 * ---------------------------------------------------------------------------------------------- */
#define LRG_BASELINE_NORMAL 0          /* normals[k].dot(normals[i]) > t1, as fma(a2,b2, fma(a1,b1, a0*b0)) in float64     */
#define LRG_BASELINE_CURVATURE 1       /* |curvatures[k] - curvatures[i]| < t1 in float64                                   */
#define LRG_BASELINE_COLOR 2           /* (d0^2 + d1^2) + d2^2 < (float)t1 in float32, d = rgb[k] - rgb[i]                 */
#define LRG_BASELINE_FEATURE 3         /* normal with t1 AND curvature with t2 AND color with (float)t3                     */
#define LRG_BASELINE_SMOOTHNESS 4      /* the normal edges; regions numbered and sized as the reference's DFS (:380-405)     */
#define LRG_BASELINE_MAX_MIN_CLUSTER 64
/* Workspace of lrg_baseline_segment: 0 when an argument is out of range (1 <= min_cluster_size <= 64). */
size_t lrg_baseline_workspace_bytes(int n_points, int n_rooms, int min_cluster_size);
/* A batch of equalised rooms in one fixed sequence of launches.  room_start [n_rooms + 1] is HOST memory: room r owns points
 * room_start[r] .. room_start[r+1]-1, room_start[0] = 0, n = room_start[n_rooms] (LRG_EINVAL - 73 if it is not non-decreasing).
 * Device pointers: pts [n, ld] float32 (xyz, rgb in columns 0-5),
 * normals [n, 3] and
 * curvatures [n] float64, rank [n] int32 = the point's position in numpy.argsort(curvatures) of its room (smoothness only).
 * normals, curvatures and rank may be NULL when the mode does not read them (LRG_EINVAL - 74 when it does).
 * labels [n] int32: 0 = no cluster, else the room's cluster id (1, 2, ... in the reference's order); n_clusters [n_rooms].
 * A component is kept when it has more than min_cluster_size points; for smoothness, when the reference's DFS pops more than
 * min_cluster_size times (duplicates included).  Errors found on the device go to lrg_baseline_status. */
int lrg_baseline_segment(const float *pts, int ld, const int32_t *room_start, int n_rooms, float resolution, int mode,
                         const double *normals, const double *curvatures, const int32_t *rank, double t1, double t2, double t3,
                         int min_cluster_size, void *ws, size_t ws_bytes, int32_t *labels, int32_t *n_clusters, void *stream);
/* Error bits of the last lrg_baseline_segment on this workspace (synchronises the stream): 1 a voxel outside the 21-bit window,
 * 2 two points of one room in one voxel (the room is not equalised), 4 a rank outside [0, room size), 8 a replay stack
 * overflow (not reachable by the bound of DESIGN.md §3.8).  Labels are not valid when it is non-zero. */
int lrg_baseline_status(const void *ws, int n_points, int n_rooms, int min_cluster_size, int32_t *host_status, void *stream);
/* ABI 11.  The features of benchmarks.py:242-246 solved on the device, with a bound on their distance from numpy.linalg.svd's (DESIGN.md
 * §3.8 "verified").  cov [n, 9] float64 as lrg_preprocess eig_mode 0 writes it, any number of rooms one after the other; one lane
 * per point runs the Jacobi solve of lrg_preprocess eig_mode 1 (same code, same selection and tie rules).  All pointers on the device:
 * normals [n, 3] = |V[smallest]|, curvatures [n] = |s2 / (s0 + s1 + s2)| (not divided by a maximum),
 * normal_slack [n] = 256 eps s0 / (s1 - s2): LAPACK's normal lies within it in every component; curv_slack [n] = 256 eps likewise.
 * Both are +inf where !(s1 - s2 > 1e-6 s0) or the curvature is NaN: no bound, the point has to go through LAPACK. */
int lrg_baseline_eig(const double *cov, int n, double *normals, double *curvatures, double *normal_slack, double *curv_slack, void *stream);
/* ABI 11.  Which points could change an edge of lrg_baseline_segment(mode, t1, t2, t3) if LAPACK's features replaced the device's?
 * The inputs of lrg_baseline_segment (rank is not read and labels are not written, so neither is passed) plus the slacks of
 * lrg_baseline_eig (0 = the value is LAPACK's own).  Every edge candidate (k < i on the 26-neighbour graph) is evaluated with the
 * segmentation's own arithmetic; a normal conjunct is certain iff |d - t| > 2 E_n, E_n = 2 (s_i + s_k) + 3 s_i s_k + 8 eps, a
 * curvature conjunct iff ||c_k - c_i| - t| > 2 E_c, E_c = sc_i + sc_k + 2 eps (NaN and infinity: uncertain), the colour conjunct
 * always.  flags [n] int32 (device) = 1 for both ends of every edge with an uncertain conjunct and none certainly false, else 0;
 * n_flagged [1] int32 (device) = their number.  After the flagged points' features are replaced by LAPACK's (slack 0) no edge can
 * differ from the all-LAPACK outcome: one pass is enough.  normal_slack / curv_slack may be NULL when the mode does not read them.
 * LRG_BASELINE_COLOR: flags and n_flagged are cleared, no kernel is launched.  Same workspace as lrg_baseline_segment (which may
 * follow on it), same lrg_baseline_status. */
int lrg_baseline_certify(const float *pts, int ld, const int32_t *room_start, int n_rooms, float resolution, int mode, const double *normals,
                         const double *curvatures, const double *normal_slack, const double *curv_slack, double t1, double t2, double t3,
                         int min_cluster_size, void *ws, size_t ws_bytes, int32_t *flags, int32_t *n_flagged, void *stream);
/* The edges of test_mcpnet.py:122-145 (MCPNet): emb[k].dot(emb[i]) > t on the 26-neighbour voxel graph, the dot a float64 sum of the
 * exact products double(emb[k][d]) * double(emb[i][d]) taken in order d = 0, 1, ..., dim - 1 ((p0 + p1) + p2 ...: what OpenBLAS's ddot
 * gives for n = 10).  emb [n, dim] float32 on the device, 1 <= dim <= 64.  Components of more than min_cluster_size
 * points are numbered in networkx's order, as the non-smoothness modes of lrg_baseline_segment; same workspace, same status. */
int lrg_baseline_segment_embedding(const float *pts, int ld, const int32_t *room_start, int n_rooms, float resolution, const float *emb,
                                   int dim, double t, int min_cluster_size, void *ws, size_t ws_bytes, int32_t *labels,
                                   int32_t *n_clusters, void *stream);
/* The edges of benchmarks.py:300-306 (modes pointnet / pointnet2): cls[k] == cls[i] on the 26-neighbour voxel graph, cls [n] int32 on
 * the device (any values: a class count is not needed).  Components of more than min_cluster_size points are numbered in networkx's
 * order (:405-416), as lrg_baseline_segment_embedding does; same workspace (lrg_baseline_workspace_bytes), same lrg_baseline_status. */
int lrg_baseline_segment_labels(const float *pts, int ld, const int32_t *room_start, int n_rooms, float resolution, const int32_t *cls,
                                int min_cluster_size, void *ws, size_t ws_bytes, int32_t *labels, int32_t *n_clusters, void *stream);
/* ABI 18.  The edges of benchmarks.py:359-367 (mode fpfh) on the 26-neighbour voxel graph: hist [n, 33] float32 on the device; in float64
 * without contraction s = the sum over d = 0 .. 32, in that order, of double(hist[d])^2, u[d] = double(hist[d]) / sqrt(s), and an edge iff
 * ((u_i[0] u_k[0] + u_i[1] u_k[1]) + ...) > t, every product and every sum rounded (a zero histogram gives NaN: no edge).  u [n, 33]
 * float64 is made once per call in the workspace, which is therefore larger than its siblings': lrg_baseline_fpfh_workspace_bytes
 * (0 when an argument is out of range).  Components and numbering as lrg_baseline_segment_embedding; the same lrg_baseline_status
 * reads this workspace too.  DESIGN.md §3.15. */
size_t lrg_baseline_fpfh_workspace_bytes(int n_points, int n_rooms, int min_cluster_size);
int lrg_baseline_segment_fpfh(const float *pts, int ld, const int32_t *room_start, int n_rooms, float resolution, const float *hist, double t,
                              int min_cluster_size, void *ws, size_t ws_bytes, int32_t *labels, int32_t *n_clusters, void *stream);

/* ABI 19.  Components of edges the caller has decided (benchmarks.py:353 edges = E[criteria], then :406-416).  The 26 offsets are numbered
 * 0 .. 25 in itertools.product([-1, 0, 1], repeat=3) order without (0, 0, 0), so that offsets o and 25 - o are opposite; the edge between a
 * point and its neighbour at offset 13 + s is bit s of the point's word in keep [n] uint32 (device), and is the only place that edge is
 * stored.  Bits of missing neighbours are not read.  Numbering, min_cluster_size, workspace and status as lrg_baseline_segment_embedding. */
int lrg_baseline_segment_mask(const float *pts, int ld, const int32_t *room_start, int n_rooms, float resolution, const uint32_t *keep,
                              int min_cluster_size, void *ws, size_t ws_bytes, int32_t *labels, int32_t *n_clusters, void *stream);

/* ------------------------------------------------------------------------------------------------
 * ABI 19.  The edge-classifier baseline, benchmarks.py --mode edge (:308-353 features, classifier and criteria, :406-436 components and
 * the fallback search; csrc/lrg_edge.hip).  Rooms as for lrg_baseline_segment: equalised, room_start in HOST memory.
 * Per-edge arrays are [n, 13] float64: slot [i, s] is the edge between i and its neighbour at offset 13 + s (numbering as
 * lrg_baseline_segment_mask), NaN where there is none; each edge of the voxel graph has exactly one slot.
 * ---------------------------------------------------------------------------------------------- */
#define LRG_EDGE_WEIGHTS 9451          /* doubles: W0 [30,100] | b0 | W1 [100,50] | b1 | W2 [50,25] | b2 | W3 [25,1] | b3, [in, out] row-major */
/* Workspace of lrg_edge_segment (lrg_edge_logits needs less and accepts it): 0 when an argument is out of range
 * (1 <= min_cluster_size <= 64, 1 <= search_cap <= 2^20). */
size_t lrg_edge_workspace_bytes(int n_points, int n_rooms, int min_cluster_size, int search_cap);
/* :325-345 up to the logit.  nmin / nmax [n, 6] float32 (device, may be NULL): minimum and maximum of columns 0-5 over the point and its
 * neighbours (:333-339).  z [n, 13] float64 (device): for every existing edge the 30 float32 features of :309-324 (mean, min, max of
 * columns 2-5; |p1 - p2| of columns 0-5; the nmin term; the nmax term; each one or two rounded float32 operations) through the four
 * layers of the reference's MLPClassifier (30-100-50-25-1, relu) in float64: acc = 0, acc = acc + x[k] * W[k][j] for k ascending with the
 * product and the sum each rounded, then + b[j], then max(., 0); the last layer's sum plus its bias is z, the value before the
 * logistic function of predict_proba (:345).  weights: LRG_EDGE_WEIGHTS float64 on the device. */
int lrg_edge_logits(const float *pts, int ld, const int32_t *room_start, int n_rooms, float resolution, const double *weights, void *ws,
                    size_t ws_bytes, double *z, float *nmin, float *nmax, void *stream);
/* p = 1 / (1 + exp(-z)) for count float64 values on the device, NaN kept.  Not bit-identical to scipy.special.expit. */
int lrg_edge_sigmoid(const double *z, long count, double *p, void *stream);
/* :346-353 and :406-436 from p [n, 13] (device, values in [0, 1] or NaN where there is no edge).  An edge is kept when
 * p > rel * pmax[i] && p > rel * pmax[k] && p > floor (:351-352: rel 0.99, floor 0.9), pmax = the maximum of 0 and the p of the point's
 * edges, the products rounded in float64.  Components of the kept edges with more than min_cluster_size points are the clusters
 * (lrg_baseline_segment_mask; n_clusters [n_rooms]).  Every unlabelled point of a voxel-graph component that holds a cluster is then
 * searched from as :424-436 does, one wavefront per search, and takes the label of the point its search stopped at.
 * Outputs (device): labels [n] int32; stop [n] int32: the point the search from i stopped at (its index in the batch), -1 where none ran (clustered points and
 * components without a cluster, whose points keep label 0), -2 where the search would have visited more than search_cap nodes (the
 * point keeps label 0, as does every point whose chain ends there: the caller finishes them); counters [4] int32: points in components
 * without a cluster, searches, searches that overflowed, the largest number of nodes a search visited (its start included);
 * keep [n] uint32 and cluster_labels [n] int32 (either may be NULL): the keep words and the labels before the fallback.
 * prepared != 0: ws is the workspace the last lrg_edge_logits ran on with these pts, room_start and resolution, and nothing else has
 * written it since; its hash, neighbour table and status are used as they stand instead of being built again.
 * Errors found on the device go to lrg_edge_status. */
int lrg_edge_segment(const float *pts, int ld, const int32_t *room_start, int n_rooms, float resolution, const double *p, double rel, double floor,
                     int min_cluster_size, int search_cap, void *ws, size_t ws_bytes, int32_t *labels, int32_t *n_clusters, int32_t *stop,
                     int32_t *counters, uint32_t *keep, int32_t *cluster_labels, int prepared, void *stream);
/* Error bits of the last lrg_edge_logits / lrg_edge_segment on this workspace (synchronises the stream): 1 a voxel outside the 21-bit
 * window, 2 two points of one room in one voxel (the room is not equalised), 4 a label chain was not resolved (not reachable: a
 * chain has fewer links than points).  The outputs are not valid when it is non-zero. */
int lrg_edge_status(const void *ws, int32_t *host_status, void *stream);

/* ------------------------------------------------------------------------------------------------
 * ABI 18.  Fast Point Feature Histograms for benchmarks.py --mode fpfh (:354-358) without PCL: the arithmetic of PCL's
 * FPFHEstimation in float32 on the +-2 voxel window of an equalised room (csrc/lrg_fpfh.hip).
 * ---------------------------------------------------------------------------------------------- */
#define LRG_FPFH_LISTS 1               /* flags: the pair pass stores each point's neighbour list for the gather pass (192 B a point) */
/* Workspace of lrg_fpfh: 0 when an argument is out of range. */
size_t lrg_fpfh_workspace_bytes(int n_points, int n_rooms, int flags);
/* A batch of equalised rooms in one fixed sequence of launches (init, insert, pairs, gather).  room_start [n_rooms + 1] is HOST memory,
 * as for lrg_baseline_segment.  Device pointers: pts [n, ld] float32, ld >= 3: columns 0-2 give the voxels (rint(x / resolution));
 * xyz [n, 3] and normals [n, 3] float32: the values every distance and pair feature is computed from (the caller's PCD round trip of
 * pts and of the normals).  A neighbour of i is every j of i's room, i included, whose voxel lies within +-2 of i's on every axis and
 * whose d2 = (dx dx + dy dy) + dz dz <= radius * radius in float32; neighbours never cross a room boundary.  radius > 2 * resolution
 * is refused with LRG_EINVAL: the window could not hold the ball.
 * Outputs (device): counts [n, 33] int32, the three 11-bin pair-feature histograms of the point; k [n] int32, its neighbour count
 * (itself included); fpfh [n, 33] float32, the distance-weighted sum of the neighbours' histograms, each block of 11 scaled to
 * sum 100.  The output does not depend on flags, on the batch or on the run.  Errors found on the device go to lrg_fpfh_status. */
int lrg_fpfh(const float *pts, int ld, const float *xyz, const float *normals, const int32_t *room_start, int n_rooms, float resolution,
             float radius, int flags, void *ws, size_t ws_bytes, int32_t *counts, int32_t *k, float *fpfh, void *stream);
/* Error bits of the last lrg_fpfh on this workspace (synchronises the stream), with the meanings of lrg_baseline_status: 1 a voxel
 * outside the 21-bit window, 2 two points of one room in one voxel.  The outputs are not valid when it is non-zero. */
int lrg_fpfh_status(const void *ws, int n_points, int n_rooms, int flags, int32_t *host_status, void *stream);

/* ------------------------------------------------------------------------------------------------
 * PointNet2's shared MLPs (train_pointnet.py:126-167, :193-202; the caller is benchmarks.py:281-298).  fp32 on
 * v_mfma_f32_32x32x2_f32; a tile of 32 rows stays on its CU from the first layer to the last (csrc/lrg_pointnet2.hip).  An output
 * value depends on its own row or group only: not on the launch's size nor on what else is in it.
 * ---------------------------------------------------------------------------------------------- */
/* Floats of one packed layer of k inputs and n outputs (1 <= k <= 1024, 1 <= n <= 512; 0 otherwise): both rounded up to a multiple of 32,
 * then the bias.  A multiple of 32 floats, so the layers of one MLP follow each other in one 16-byte aligned buffer. */
size_t lrg_pointnet2_packed_floats(int k, int n);
/* One 1x1 convolution (:133-136, :161-164, :194-202): w [k, n] row-major (the TF kernel [1,1,k,n] or [1,k,n]) and bias [n] on the device
 * -> packed [lrg_pointnet2_packed_floats(k, n)] in the MFMA operand order, zero where padded.  The packed image of an MLP is its layers'
 * images one after the other. */
int lrg_pointnet2_pack_layer(int k, int n, const float *w, const float *bias, float *packed, void *stream);
/* A set-abstraction level after its ball query (pointnet_sa_module, :126-140, with the grouping of sample_and_group :116-122): for every
 * group g of batch element bi, the 32 rows concat(xyz[bi][idx[g][s]] - new_xyz[g], points[bi][idx[g][s]]) (float32 subtraction; never
 * written to memory), three layers relu(x W + bias) of widths[0..2] (HOST memory; each a multiple of 32, at most 512), then the
 * maximum over the 32 rows: out [b, m, widths[2]].  xyz [b,n,3], new_xyz [b,m,3], points [b,n,c] (NULL with c == 0; 3 + c <= 1024),
 * idx [b,m,32] int32 (an index outside [0, n) reads row 0).  nsample must be 32: one MFMA row tile is one group. */
int lrg_pointnet2_group_mlp(int b, int n, int m, int nsample, int c, const float *xyz, const float *new_xyz, const float *points,
                            const int32_t *idx, const int32_t *widths, const float *packed, float *out, void *stream);
/* The layers of pointnet_fp_module after its interpolation (:152-166) and the head (:193-202): rows concat(a[i], b[i]) (a [r, ca],
 * b [r, cb], NULL with cb == 0; ca + cb <= 1024; the concat of :153 is never written), n_layers (1 .. 3) layers x W + bias of
 * widths[0 .. n_layers-1] (HOST memory; at most 512; all but the last a multiple of 32, the last any value from 1), ReLU after each
 * layer except that relu_last == 0 leaves it off the last: out [r, widths[n_layers-1]].  r >= 0. */
int lrg_pointnet2_row_mlp(long r, int ca, int cb, const float *a, const float *b, int n_layers, const int32_t *widths, int relu_last,
                          const float *packed, float *out, void *stream);
/* The two entry points above in the training forward (ABI 17): the same arguments, the same checks and error codes, bit for bit the
 * same `out`, and besides it what the backward pass reads, each pointer nullable (NULL: not written):
 *   rows  [b*m*32, 3 + c]      the grouped rows concat(xyz[idx] - new_xyz, points[idx]) that group_point and the concat of
 *                              sample_and_group (:116-120) would have written;
 *   keepL [rows, widths[L]]    layer L's output after its ReLU (:137, :165), unpadded; for the grouped form keep2 is the last layer
 *                              BEFORE the maximum over the 32 rows ([b*m*32, widths[2]]); for the row form keepL with L == n_layers-1
 *                              repeats `out` and keepL with L >= n_layers is ignored. */
int lrg_pointnet2_group_mlp_train(int b, int n, int m, int nsample, int c, const float *xyz, const float *new_xyz, const float *points,
                                  const int32_t *idx, const int32_t *widths, const float *packed, float *out, float *rows, float *keep0,
                                  float *keep1, float *keep2, void *stream);
int lrg_pointnet2_row_mlp_train(long r, int ca, int cb, const float *a, const float *b, int n_layers, const int32_t *widths, int relu_last,
                                const float *packed, float *out, float *keep0, float *keep1, float *keep2, void *stream);

/* ------------------------------------------------------------------------------------------------
 * The plain PointNet of benchmarks.py --mode pointnet (train_pointnet.py:31-99) at inference (ABI 15; csrc/lrg_pointnet.hip).  A cell
 * is 1024 rows.  fp32 on v_mfma_f32_32x32x2_f32; a tile of 32 rows stays on its CU through the conv stack, and again through the fc
 * stack.  A cell's values depend on that cell only: not on the launch's size nor on what else is in it.  No entry point allocates.
 * ---------------------------------------------------------------------------------------------- */
/* lrg_pointnet2_packed_floats / lrg_pointnet2_pack_layer with the caps 1 <= k <= 2048, 1 <= n <= 1024 (the same image). */
size_t lrg_pointnet_packed_floats(int k, int n);
int lrg_pointnet_pack_layer(int k, int n, const float *w, const float *bias, float *packed, void *stream);
/* :49-56.  x [cells,1024,6] through n_conv (2 .. 5) layers relu(x W + bias) of widths[0 .. n_conv-1] (HOST memory; each a multiple of
 * 32, at most 1024); packed: the layers' images one after the other, the first with k = 6.  skip [cells,1024,widths[1]] receives
 * conv[1], last [cells,1024,widths[n_conv-1]] the last layer's rows (NULL: not written), pooled [cells,widths[n_conv-1]] the column
 * maximum over ALL 1024 rows of the cell (an integer maximum on the bits of the non-negative values: the same bits in any order; the
 * entry point zeroes pooled on the stream first).  cells >= 0. */
int lrg_pointnet_features(int cells, int n_conv, const int32_t *widths, const float *x, const float *packed, float *skip, float *last,
                          float *pooled, void *stream);
/* :57-99.  Rows concat(last[p] - pooled[cell] (float32), skip[p]) (never written; c_last, c_skip multiples of 32 up to 1024, their
 * sum at most 1248), n_fc (2 .. 3) layers of widths[0 .. n_fc-1] (HOST memory): the hidden ones (multiples of 32 up to 512) are
 * relu((x W + bias) * scale[p][c] + shift[p][c]) with p = 0 .. 1023 the row's position in its cell, the last (1 .. 1024 classes) is
 * x W + bias: out [cells,1024,widths[n_fc-1]].  bn: for every hidden layer j in turn scale [1024, widths[j]] then shift
 * [1024, widths[j]], the batch norm of :63-84 folded as tf.nn.batch_normalization does (scale = rsqrt(var + 1e-3) * gamma,
 * shift = beta - mean * scale). */
int lrg_pointnet_head(int cells, int c_last, int c_skip, const float *last, const float *skip, const float *pooled, int n_fc,
                      const int32_t *widths, const float *packed, const float *bn, float *out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * MCPNet (test_mcpnet.py:71-120, learn_region_grow_util.py:191-225): candidate lists on 0.3 m cells, 50 neighbour rows per point,
 * the embedding network.  extern "C"; int return; no entry point allocates.  DESIGN.md §3.9.
 * ---------------------------------------------------------------------------------------------- */
#define LRG_MCP_NEIGHBORS 50            /* num_neighbors (test_mcpnet.py:19)                                                  */
#define LRG_MCP_RADIUS 0.3f             /* neighbor_radii (test_mcpnet.py:20): cells round(x / 0.3f) in float32, half to even   */
#define LRG_MCP_HIDDEN 200
#define LRG_MCP_EMBEDDING 10
/* Workspace of lrg_mcp_candidates / lrg_mcp_neighbors: 0 when an argument is out of range (n_rooms >= 1). */
size_t lrg_mcp_workspace_bytes(int n_points, int n_rooms);
/* The candidate lists of a batch of centred, equalised rooms (test_mcpnet.py:75-104): the members of the 27 cells around a point's
 * own cell, cells in itertools.product order (dz fastest), members in ascending index, the point included.  room_start as for
 * lrg_baseline_segment (HOST memory); pts [n, ld] on the device; counts [n] int32: the candidate count of every point. */
int lrg_mcp_candidates(const float *pts, int ld, const int32_t *room_start, int n_rooms, void *ws, size_t ws_bytes, int32_t *counts,
                       void *stream);
/* nbr [n, 50] int32 (global point indices) from the workspace lrg_mcp_candidates left, same pts and room_start
 * (test_mcpnet.py:104, numpy.random.choice(neighbors, 50, replace=len(neighbors) < 50)):
 *   positions != NULL (legacy)  positions [n, 50] int32 on the device, each in [0, count): drawn on the host; mapped here
 *   positions == NULL (counter) Philox4x32-10 keyed by (seed, room_ids[r]) (room_ids HOST memory), counter (j / 4, 0, point index in
 *                               the room, LRG_PURPOSE_MCP_NEIGHBOR): count >= 50 the first 50 of a Feistel permutation of
 *                               [0, count), else 50 independent (w * count) >> 32. */
int lrg_mcp_neighbors(const float *pts, int ld, const int32_t *room_start, int n_rooms, void *ws, size_t ws_bytes,
                      const int32_t *positions, uint32_t seed, const int32_t *room_ids, int32_t *nbr, void *stream);
/* Error bits of the last lrg_mcp_candidates / lrg_mcp_neighbors on this workspace (synchronises the stream): 1 a cell outside the
 * 21-bit window, 2 a legacy position outside [0, count). */
int lrg_mcp_status(const void *ws, int n_points, int n_rooms, int32_t *host_status, void *stream);
/* Floats of the packed weights lrg_mcp_embed reads. */
size_t lrg_mcp_packed_floats(void);
/* The eight mcp_* trainables (device, TF layouts: kernel1 [1,6,200], bias1 [200], kernel2 [1,200,200], bias2 [200], kernel3 [204,200],
 * bias3 [200], kernel4 [200,10], bias4 [10]) -> packed [lrg_mcp_packed_floats()] in the operand order of lrg_mcp_embed. */
int lrg_mcp_pack_weights(const float *k1, const float *b1, const float *k2, const float *b2, const float *k3, const float *b3,
                         const float *k4, const float *b4, float *packed, void *stream);
/* emb [n, 10] float32 (learn_region_grow_util.py:210-225) for pts [n, ld] (ld >= 6) and nbr [n, 50]: rows points[nbr] - points[i]
 * (all six columns), relu(. K1 + b1), relu(. K2 + b2) on v_mfma_f32_32x32x2_f32, max over the 50 rows, concat(points[i, 2:6], .),
 * relu(. K3 + b3), . K4 + b4, l2_normalize.  One launch.  *status (device int32) gets bit 1 when a neighbour index is outside
 * [0, n) (that row then uses the point itself). */
int lrg_mcp_embed(const float *pts, int ld, int n_points, const int32_t *nbr, const float *packed, float *emb, int32_t *status,
                  void *stream);

/* ---- training MCPNet (ABI 20; train_mcpnet.py, metric_loss_ops.py:40-81 and :119-236; csrc/lrg_mcpnet_train.hip) ---- */
#define LRG_MCP_TRAIN_POINTS 2   /* points per workgroup of lrg_mcp_embed_train */
#define LRG_MCP_TRIPLET_MAX_B 1024
/* lrg_mcp_embed with every layer kept (learn_region_grow_util.py:210-225 as train_mcpnet.py:197 runs it): x [n, 50, 6] the staged
 * rows (already the float32 differences neighbour - point), c [n, 4] the centre features (z, r, g, b), packed as lrg_mcp_pack_weights
 * left it.  h1, h2 [n * 50, 200] (after ReLU), cat [n, 204], fc3 [n, 200], fc4 [n, 10], emb [n, 10]; any of h1, h2, cat, fc3, fc4 may
 * be NULL (all NULL: the validation forward).  emb carries the bits lrg_mcp_embed gives for points whose differences are x. */
int lrg_mcp_embed_train(const float *x, const float *c, int n, const float *packed, float *h1, float *h2, float *cat, float *fc3,
                        float *fc4, float *emb, void *stream);
/* Doubles of the workspace of lrg_mcp_triplet_semihard for a batch of B. */
size_t lrg_mcp_triplet_workspace_doubles(int B);
/* triplet_semihard_loss (metric_loss_ops.py:157-236, pairwise_distance(squared=True) :40-81) of emb [B, 10] = l2_normalize(fc4 [B, 10])
 * with labels [B] (int32, any values), 2 <= B <= LRG_MCP_TRIPLET_MAX_B, and its gradient by TensorFlow's registered rules:
 *   D [B, B]     max((sq_i + sq_j) - 2 dot_ij, 0), diagonal 0; sq and dot summed over the 10 columns in ascending order, products
 *                rounded (no FMA)
 *   dD [B, B]    d(loss)/d(squared distance before the clamp): zero on the diagonal and where D <= 0
 *   dfc4 [B, 10] dE_i = 2 sum_j (dD_ij + dD_ji)(e_i - e_j) in ascending j, then l2_normalize's backward
 *   stats [4]    doubles: the loss numerator, num_positives, the positive pairs with a gradient (margin + D_ap - S_ap >= 0), the
 *                positive pairs that took negatives_inside
 * Nothing is added atomically: the same inputs give the same bits.  ws: lrg_mcp_triplet_workspace_doubles(B) doubles.
 * LRG_EINVAL - 91: B outside the range (nothing is launched). */
int lrg_mcp_triplet_semihard(const float *fc4, const float *emb, const int32_t *labels, int B, float margin, float *D, float *dD,
                             float *dfc4, double *stats, double *ws, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Training side: the pieces of the backward pass and of AdamOptimizer
 * (learn_region_grow_util.py:165-189) that the forward entry points do not cover.  The step is sequenced by the host
 * mirror (learn_region_grow_amd/train.py: LrgNetTrainer.train_step = sess.run([net.train_op, net.loss, ...]) at
 * train_region_grow.py:175).
 * ---------------------------------------------------------------------------------------------- */
/* C[M,N] = op(A)[M,K] op(B)[K,N] in fp32 on the matrix cores.  transA: A is stored [K,M] (row stride lda), else [M,K];
 * transB: B is stored [N,K] (row stride ldb), else [K,N].  Epilogue: C = acc + addend (nullable, [M,N] with row stride ldc),
 * then C = 0 where mask <= 0 (nullable, same shape: the ReLU gradient of the layer whose output the result is the gradient of).
 * split_k > 1: the reduction is split over that many workgroup layers which ADD into C -- the caller zeroes C first, and no
 * epilogue is allowed.  dX = dZ W^T is (transB = 1); dW = X^T dZ over all rows is (transA = 1, split_k ~ rows / 1024). */
int lrg_gemm_f32(int M, int N, int K, const float *A, int lda, int transA, const float *B, int ldb, int transB, float *C, int ldc,
                 const float *addend, const float *mask, int split_k, void *stream);
/* The same product with the reduction split WITHOUT atomics (ABI 16): slice z of K stores its partial product in
 * planes[z] ([M,N], row stride N; every element of every plane is written), z < lrg_gemm_f32_planes_count(K, split_k) <= split_k.
 * The caller adds the planes in a fixed order (lrg_segment_colsum(planes, 1, count, M * N, out)), so that the same inputs give the
 * same bits.  LRG_EINVAL - 2: more than 65535 planes. */
int lrg_gemm_f32_planes_count(int K, int split_k);
int lrg_gemm_f32_planes(int M, int N, int K, const float *A, int lda, int transA, const float *B, int ldb, int transB, float *planes,
                        int split_k, void *stream);
/* d(loss)/d(logits) of a sparse softmax cross entropy over `rows` two-class slots with per-class weights
 * (add head :174: w_pos = w_neg = 1 / rows; remove head :166-172: 1 / #positive and 1 / #negative slots of the batch).
 * stats (device double[8], ACCUMULATED): 0 weighted loss, 1 slots with argmax == label, 2 true positives, 3 predicted
 * positives, 4 labelled positives, 5 rows (the numerators of add_acc, add_prc, add_rcl ... at :175-184).  The weighted loss
 * of a call is summed in a fixed order: the same inputs add the same bits. */
int lrg_ce_grad(const float *logits, const int32_t *labels, long rows, float w_pos, float w_neg, float *dlogits, double *stats,
                void *stream);
/* lrg_ce_grad with the remove head's class weights (learn_region_grow_util.py:166-172) taken on the device (ABI 24): n_pos = the sum of
 * positives [n_counts] (int32, e.g. lrg_train_assemble's per-instance sums), w_pos = n_pos ? (float)(1.0 / (double)n_pos) : 0,
 * w_neg the same with rows - n_pos -- the values train.py hands lrg_ce_grad from the host, so dlogits and stats have the same bits and
 * the step reads nothing back.  LRG_EINVAL - 1: a NULL pointer or rows <= 0; - 2: n_counts < 1. */
int lrg_ce_grad_counted(const float *logits, const int32_t *labels, long rows, const int32_t *positives, int n_counts, float *dlogits,
                        double *stats, void *stream);
/* Gradient of the column max over each instance's rows (:122-123) followed by the pooled layer's ReLU: y [B,rows,C] is that
 * layer's output, dpool [B, dpool_stride] the gradient of its column maxima; dy [B,rows,C] gets dpool / (number of rows that tie
 * for the maximum) on those rows -- tf.reduce_max's rule -- and 0 elsewhere (and 0 everywhere when the maximum is 0). */
int lrg_pool_backward(const float *y, const float *dpool, int B, int rows, int C, int dpool_stride, float *dy, void *stream);
/* out[s, n] = sum of x[s*seg_rows + r, n] over r < seg_rows, for s < n_seg (bias gradients, the gradient of the tiled pooled
 * feature: the sum over an instance's rows). */
int lrg_segment_colsum(const float *x, long n_seg, int seg_rows, int N, float *out, void *stream);
/* One AdamOptimizer update of n parameters as TensorFlow 1 applies it (:188): m += (g - m)(1 - beta1); v += (g^2 - v)(1 - beta2);
 * p -= lr_t m / (sqrt(v) + epsilon), with lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t) computed by the caller. */
int lrg_adam_step(float *params, const float *grads, float *m, float *v, long n, float lr_t, float beta1, float beta2, float epsilon,
                  void *stream);

/* ------------------------------------------------------------------------------------------------
 * Training side of the plain PointNet (train_pointnet.py:31-111; ABI 16; csrc/lrg_pointnet_train.hip): what its step needs beyond
 * lrg_gemm_f32, lrg_pointwise_layer, lrg_segmax, lrg_segment_colsum and lrg_adam_step.  The step is sequenced by
 * learn_region_grow_amd/pointnet_train.py (PointNetTrainer.train_step = sess.run([class_acc, class_loss, train_op]) at :408).
 * A cell is 1024 rows.  No entry point allocates; none uses an atomic: every sum runs in one fixed order (the batch axis in ascending
 * cell order), so the same inputs give the same bits.  Errors: LRG_EINVAL - 1 a NULL pointer, - 2 a size out of range, - 3 as noted.
 * ---------------------------------------------------------------------------------------------- */
/* :63-93 with is_training True.  z [cells,1024,c], gamma [c], beta [c]; c a multiple of 32 up to 512, cells >= 1.
 * mean [1024,c] = the mean of z over the cells; var [1024,c] = the mean over the cells of (z - mean)^2 (tf.nn.moments :70: biased,
 * two passes; exactly 0 for cells == 1); inv = rsqrt(var + 1e-3) * gamma; y = relu(z * inv + (beta - mean * inv))
 * (tf.nn.batch_normalization :83 and the ReLU of :93). */
int lrg_pointnet_bn_forward(const float *z, const float *gamma, const float *beta, int cells, int c, float *y, float *mean, float *var,
                            void *stream);
/* Bytes of lrg_pointnet_bn_backward's workspace (2 * 1024 * c floats); 0 when c is out of range. */
size_t lrg_pointnet_bn_backward_workspace_bytes(int c);
/* The gradient of :83-93 (batch norm in training mode, then ReLU).  z, y, dy [cells,1024,c]; mean, var [1024,c] as
 * lrg_pointnet_bn_forward left them.  With g = dy where y > 0 else 0, rstd = rsqrt(var + 1e-3), xhat = (z - mean) * rstd:
 * dz = gamma * rstd * (g - mean_cells(g) - xhat * mean_cells(g * xhat)) per (row position, channel); dbeta [c] and dgamma [c] are the
 * sums of g and of g * xhat over cells and rows: over the cells first (workspace), then over the 1024 row positions in a second,
 * fixed-order stage.  dz may be dy.  cells == 1 gives dz == +0 everywhere.  LRG_EINVAL - 3: the workspace is too small. */
int lrg_pointnet_bn_backward(const float *z, const float *y, const float *dy, const float *mean, const float *var, const float *gamma, int cells,
                             int c, float *dz, float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes, void *stream);
/* :102-105.  logits [rows,classes], labels [rows] int32; 1 <= classes <= 1024 (LRG_EINVAL - 3 otherwise).
 * dlogits [rows,classes] = (softmax - onehot) / rows (tf.reduce_mean of the rows' losses); NULL: not computed (evaluation).
 * stats (device double[3], ACCUMULATED): 0 the sum of the rows' losses (one fixed order), 1 the rows whose argmax is the label (a tie
 * to the lowest class, tf.argmax :104), 2 the rows whose label is outside [0, classes): such a row adds no loss, gets a zero gradient
 * row and is never used as an index. */
int lrg_pointnet_softmax_ce_grad(const float *logits, const int32_t *labels, long rows, int classes, float *dlogits, double *stats, void *stream);
/* :56-59.  t [cells,1024,c_last] = last - pooled[cell] (float32), the first block of the head's input; the second is conv[1] (:60).
 * c_last a multiple of 32 up to 1024. */
int lrg_pointnet_head_input(const float *last, const float *pooled, int cells, int c_last, float *t, void *stream);
/* The gradient of :56-59 with respect to conv_last, given dt [cells,1024,c_last]: dlast = dt, and -S[cell,c], S = the sum of dt over
 * the cell's rows, is added on the FIRST row (lowest index) of the cell whose value equals pooled[cell,c] -- the single winner of
 * tf.nn.max_pool2d's gradient (lrg_pool_backward shares among ties, tf.reduce_max's rule).  addend (nullable, the same shape) is
 * added: a second gradient of the same tensor.  relu != 0 then zeroes the result where last <= 0 (the last convolution's own ReLU).
 * dlast may be dt.  cells <= 65535. */
int lrg_pointnet_head_input_backward(const float *last, const float *pooled, const float *dt, const float *addend, int cells, int c_last,
                                     int relu, float *dlast, void *stream);
/* ExponentialMovingAverage.apply (:71-78) on n floats: shadow -= (shadow - value) * one_minus_decay. */
int lrg_pointnet_ema_update(float *shadow, const float *value, long n, float one_minus_decay, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Training side of PointNet2 (train_pointnet.py:113-211; ABI 17; csrc/lrg_pointnet2_train.hip): what its step needs beyond
 * lrg_pointnet2_*_mlp_train, lrg_three_nn_interpolate, lrg_pool_backward, lrg_gemm_f32, lrg_gemm_f32_planes, lrg_segment_colsum,
 * lrg_pointnet_softmax_ce_grad and lrg_adam_step.  The step is sequenced by learn_region_grow_amd/pointnet2_train.py
 * (PointNet2Trainer.train_step = sess.run([class_acc, class_loss, train_op])).  DESIGN.md §3.14.
 * ---------------------------------------------------------------------------------------------- */
/* The gradients of group_point (groupPointGradLauncher, tf_grouping_g.cu:61-78, :137) and of three_interpolate
 * (threeinterpolate_grad_cpu, tf_interpolate.cpp:131-155) WITHOUT atomic additions, in place of lrg_group_point_grad and
 * lrg_three_interpolate_grad inside a training step:
 *   out[bi, idx[bi, e], k] = addend[bi, idx[bi, e], k] + sum over e of weight[bi, e] * grad[bi, e / per, col0 + k],   k < c,
 * the sum over the entries e (0 <= e < q * per) that name the same source row taken in ASCENDING e from 0 (float32 multiplication, then
 * float32 addition), whatever the launch holds besides: the same inputs give the same bits.  grad [b, q, ldg] (col0 + c <= ldg: a column
 * block of a wider tensor is read in place), idx [b, q * per] int32, weight [b, q * per] (NULL: 1, no multiplication), out [b, n, c];
 * addend and mask [b, n, c], both nullable; addend may be out.  Every row of out is written: a row nobody names gets 0, or the addend
 * alone.  With mask, out = 0 where mask <= 0 (the ReLU of the layer whose output `out` is the gradient of), as lrg_gemm_f32's epilogue.
 * An index outside [0, n) follows the forward op: drop_out_of_range == 0 sends it to row 0 (lrg_pointnet2_group_mlp reads row 0),
 * 1 drops it (lrg_three_interpolate adds 0).
 *   group_point's gradient     q = m * 32, per = 1, weight NULL, col0 = 3 on the first layer's dX [b, m * 32, 3 + c], drop 0
 *   three_interpolate's        q = the queries, per = 3, weight the interpolation weights, col0 = 0, drop 1
 * q * per <= 16384 (the element's inverse lists are built in LDS); b <= 65535.  Errors: LRG_EINVAL - 1 a NULL pointer, - 2 a size out of
 * range (nothing is launched).  b == 0 returns 0. */
int lrg_pointnet2_scatter_grad(int b, int n, int q, int per, int c, const float *grad, int ldg, int col0, const int32_t *idx,
                               const float *weight, int drop_out_of_range, const float *addend, const float *mask, float *out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Room preprocessing P0 (replaces the per-room block test_region_grow.py:119-173: equalisation, per-point PCA normals and
 * curvature, feature stack).  SURVEY.md section 8f, row f1.
 *
 * raw [n_raw, raw_stride >= 6] float32 rows (x y z r g b ...), obj_id / cls_id [n_raw] (nullable).  Outputs (device,
 * capacity n_raw rows): equalized_idx [N] = raw index of the first point of every resolution-sized voxel, in file order
 * (:127-129,:134); unequalized_idx [n_raw] = equalised row of each raw point (:130); *n_equalized (device int32) = N.
 * eig_mode 0: cov [N,9] float64 = the covariance of :157, bit-identical to the NumPy loop (same neighbour and summation
 *             order); the host finishes with numpy.linalg.svd exactly as the reference does.  points may be NULL.
 * eig_mode 1: also points [N,feature_size] float32 (:165-172), obj_out / cls_out [N], curvatures [N] float64 (:163), with the
 *             3x3 decompositions done here by Jacobi iteration in float64 (agrees with LAPACK to ~1e-16 |cov|).
 * eig_mode 2: eig_mode 1 prepared for an exact finish on the host (learn_region_grow_amd.preprocess_gpu, eig='exact'): cov is written too,
 *             curvatures stay UN-normalised (S[2]/sum(S), :160-161 -- the division by the maximum, :163, is the host's, with LAPACK's own
 *             maximum), and lrg_preprocess_unsafe_normals tells which points' float32 normals are not certain to equal what
 *             numpy.linalg.svd would give (near-degenerate eigenvalue pairs, components next to a float32 rounding boundary): the host
 *             redoes those few with LAPACK and gets the reference's features and seed order bit for bit at the all-GPU rate.
 * workspace: lrg_preprocess_workspace_bytes(n_raw) bytes, 256-byte aligned.  Points whose voxel falls outside a 21-bit
 * window per axis are reported by lrg_preprocess_status (1) and left out.
 * These entries are lrg_preprocess_batch (below) with one room: the same launches, nothing copied from host memory, everything on the
 * stream.  Always size the workspace with lrg_preprocess_workspace_bytes: it is the batch's for one room (4 n_raw + 64 hash slots, the
 * batch's per-point arrays), 0 for n_raw <= 0 and for a room past the batch's limits (n_raw >= 2^30 or 4 n_raw + 64 >= 2^31:
 * lrg_preprocess then returns LRG_EINVAL - 51). */
size_t lrg_preprocess_workspace_bytes(int n_raw);
int lrg_preprocess(const float *raw, int raw_stride, const int32_t *obj_id, const int32_t *cls_id, int n_raw, float resolution,
                   int feature_size, int eig_mode, void *workspace, size_t workspace_bytes, float *points, int32_t *obj_out,
                   int32_t *cls_out, double *curvatures, int32_t *equalized_idx, int32_t *unequalized_idx, double *cov,
                   int32_t *n_equalized, void *stream);
int lrg_preprocess_status(const void *workspace, int n_raw, int32_t *host_status, void *stream);
/* after lrg_preprocess(..., eig_mode 2, ...) on this workspace: flags_out [n_equalized] int32 (device), 1 = redo this point's decomposition with LAPACK */
int lrg_preprocess_unsafe_normals(const void *workspace, int n_raw, int n_equalized, int32_t *flags_out, void *stream);
/* ABI 12.  The same block (test_region_grow.py:119-173) for all rooms of a file in one pass: a fixed number of launches whatever n_rooms
 * is.  raw [sum M, raw_stride] holds the rooms' rows one after the other, obj_id / cls_id likewise; raw_start [n_rooms + 1] is HOST memory
 * (raw_start[0] = 0, strictly increasing: an empty room is refused), copied to the workspace on the stream.  Every room has a hash table
 * and scalars of its own -- equal voxel coordinates in two rooms never meet -- and every per-room result has the bits of that room
 * alone.  Outputs as lrg_preprocess's, concatenated in room order: the equalised rows of room r are
 * eq_start[r] .. eq_start[r + 1] (eq_start [n_rooms + 1] int32, device) of points / obj_out / cls_out / curvatures / cov / equalized_idx /
 * unsafe_flags, all sized for sum M rows; equalized_idx and unequalized_idx [sum M] are room-relative.  unsafe_flags (eig_mode 2: what
 * lrg_preprocess_unsafe_normals copies out; may be NULL otherwise).  Refused with a code of their own: n_rooms < 1 or a bad raw_start[0]
 * (LRG_EINVAL - 60), a decreasing raw_start (- 61), an empty room (- 62), sum M >= 2^30 (- 63), 4 sum M + 64 n_rooms >= 2^31 (- 64: the
 * rooms' hash segments, an upper bound of their summed capacities, are numbered in int32), a NULL among raw / workspace / equalized_idx /
 * unequalized_idx / eq_start (- 65), a short or unaligned workspace (- 66), eig_mode 2 without unsafe_flags (- 67); nothing is launched. */
size_t lrg_preprocess_batch_workspace_bytes(const int32_t *raw_start, int n_rooms);     /* test_region_grow.py:119-173; 0 = bad raw_start */
int lrg_preprocess_batch(const float *raw, int raw_stride, const int32_t *obj_id, const int32_t *cls_id, const int32_t *raw_start,
                         int n_rooms, float resolution, int feature_size, int eig_mode, void *workspace, size_t workspace_bytes,
                         float *points, int32_t *obj_out, int32_t *cls_out, double *curvatures, int32_t *equalized_idx,
                         int32_t *unequalized_idx, double *cov, int32_t *eq_start, int32_t *unsafe_flags, void *stream);
/* test_region_grow.py:119-173, the batch's lrg_preprocess_status: host_status_per_room [n_rooms] (host), 1 = a point of that room lies
 * outside the voxel window (it was left out; the room's outputs are not valid).  Synchronises the stream. */
int lrg_preprocess_batch_status(const void *workspace, const int32_t *raw_start, int n_rooms, int32_t *host_status_per_room, void *stream);

/* ------------------------------------------------------------------------------------------------
 * ABI 13.  The evaluation block that follows a labelled room (test_region_grow.py:319-355, test_mcpnet.py:146-170: greedy IoU > 0.5
 * matching, PRC / RCL / mean best IoU, the relabelled clusters, and what sklearn's NMI / AMI / ARS are made of) for all rooms of a call in
 * one pass: a fixed number of launches whatever n_rooms is, everything on the stream, nothing allocated.
 *
 * Device inputs, the rooms one after the other: labels [sum N] = each room's cluster_label (0 = none, 1 .. C_r); gt_row [sum N] = the row of
 * each point's ground-truth instance (the return_inverse of numpy.unique(obj_id)); order [sum G] = per room the order in which the GT rows
 * are visited (numpy.argsort(count)[::-1] at test_region_grow.py:327, set(obj_id) order at test_mcpnet.py:152 -- the host's, because both are
 * NumPy / Python behaviour); relabel [sum G] = the value a cluster matched at visit k receives (k + 1, or the instance's id);
 * unmatched_base [n_rooms] = obj_id.max() (:339-341).  HOST arrays, copied on the stream: room_start [n_rooms + 1] and gt_start [n_rooms + 1]
 * (both begin at 0 and increase strictly: room r has N_r = room_start[r + 1] - room_start[r] points and G_r GT rows), n_cluster [n_rooms] = C_r.
 * flags bit 0: leave out the scores' float sums (the analogue of with_sklearn=False).
 *
 * Outputs (device): cluster_label2 [sum N] (matched cluster -> relabel[k], unmatched cluster j -> j + unmatched_base, 0 -> 0); best_iou
 * [sum G] float64 in visit order, with the host's bits (IEEE division of exact integers); dt_match [sum C] uint8; gt_match [n_rooms];
 * int_sums [n_rooms, 8] int64 = sum nij^2, sum a^2, sum b^2 (the adjusted Rand score's, finished in wide integers by the host), the points
 * counted, the non-empty rows, the non-empty columns (label 0 included when it occurs -- what numpy.unique keeps), the EMI's terms and its
 * chunks; float_sums [n_rooms, 4] float64 = H(true), H(pred), the mutual information before sklearn's clip at 0, and the expected mutual
 * information (sklearn's entropy, mutual_info_score and _expected_mutual_info_fast.pyx term by term over one lgamma table 0 .. max N), zero
 * with flags bit 0.  No floating-point atomics: every float64 sum is made of partials whose bounds depend on the room alone, added in a
 * fixed order, so a room's outputs are the same bits in any batch and from run to run.
 *
 * A label outside [0, C_r] or a gt_row outside [0, G_r) is skipped and raises bit 0 of the room's status word (bit 1: an `order` entry
 * outside [0, G_r)); nothing is written out of bounds, the other rooms are not affected.  lrg_metrics_batch_status copies the words to
 * host_status_per_room [n_rooms] (host) and synchronises the stream.
 *
 * Limits: at most 65536 rooms; sum N, sum G, sum (C_r + 1) and the table cells sum G_r (C_r + 1) each below 2^30; at most 2^24 table cells
 * per room; the EMI's chunk numbering, sum over the rooms of G_r (C_r + 1) + min(G_r, C_r + 1) N_r / 32 + 1, below 2^31 - 256.  Tables of up
 * to 8192 cells are counted in LDS, larger ones with global integer atomics (the same bits).
 * Refused with a code of their own, nothing launched: n_rooms out of range, a NULL host array or a start that does not begin at 0
 * (LRG_EINVAL - 90), a decreasing start (- 91), an empty room or a room without a GT row (- 92), a negative n_cluster (- 93), a sum past
 * the limits above (- 94), a NULL among the device pointers / workspace / outputs (- 95), a short or not 256-byte aligned workspace (- 96).
 * lrg_metrics_batch_workspace_bytes is host-only arithmetic and returns 0 for arguments the call would refuse. */
size_t lrg_metrics_batch_workspace_bytes(const int32_t *room_start, const int32_t *gt_start, const int32_t *n_cluster,
                                         int n_rooms);     /* test_region_grow.py:319-355, test_mcpnet.py:146-170 */
/* test_region_grow.py:319-355, test_mcpnet.py:146-170 */
int lrg_metrics_batch(const int32_t *labels, const int32_t *gt_row, const int32_t *order, const int32_t *relabel, const int32_t *unmatched_base,
                      const int32_t *room_start, const int32_t *gt_start, const int32_t *n_cluster, int n_rooms, unsigned flags,
                      void *workspace, size_t workspace_bytes, int32_t *cluster_label2, double *best_iou, uint8_t *dt_match,
                      int32_t *gt_match, int64_t *int_sums, double *float_sums, void *stream);
/* test_region_grow.py:319-355, test_mcpnet.py:146-170: the per-room status words of the last lrg_metrics_batch on this workspace. */
int lrg_metrics_batch_status(const void *workspace, const int32_t *room_start, const int32_t *gt_start, const int32_t *n_cluster, int n_rooms,
                             int32_t *host_status_per_room, void *stream);

/* ------------------------------------------------------------------------------------------------
 * ABI 22.  Training tuples for LrgNet (stage_data.py:104-240) on the device, under the counter stream (csrc/lrg_rng.h: key (rng_seed,
 * LrgRoom.room_id), purposes STAGE_SEED 5 .. STAGE_NEIGHBOR 10; a build extension as in the grow loop -- the reference draws from one
 * legacy stream).  Of LrgRoom the calls read points, voxels, obj_id, n and room_id and write visited.
 *
 * lrg_stage_teacher: one workgroup per entry of room_list [n_list] (indices into `rooms`), all in one launch; no workgroup waits for
 * another.  It runs the loop of stage_data.py:104-231 for the room: the seed order is the Feistel permutation of the room's points; per
 * object the mistake probabilities, per pass the candidates (inside the dilated box, neither current nor visited) and the current points,
 * both in point-index order, the teacher's decisions, the stuck flag, the rule that a removal which would empty the mask is skipped
 * (:213), the new box, completion, early termination, cluster_threshold and `visited`.  It emits no float rows.  Room r works in
 * cur_mask [ws_off[r] ..) (n bytes), lists [2 ws_off[r] ..) (2 n words) and objects [4 ws_off[r] ..) (4 n words), and writes into its
 * arena, arena [arena_off[r] .. + arena_cap[r]) words: list entries from the front (a point index, bit 31 = its remove / add flag),
 * 8-word tuple headers from the back (tuple k at arena_cap - 8 (k + 1): inlier count, neighbour count, offsets of both lists in the
 * room's arena, `complete` = (float)((double)inter / (double)union) as bits, the object's seed, the pass, 0).  A side of more than
 * max_points entries is emitted as its Feistel subset, and the "continue growing" test of :209 then looks at the emitted flags (:182,
 * :192).  Per stored object: objects [4 ws_off[r] + 4 j ..) = steps, seed, points of the final mask, its IoU as float bits.
 * status [4 r ..) = LRG_STAGE_OK / LRG_STAGE_OVERFLOW (a tuple would overrun the arena: the room stopped there; run it again with a
 * larger arena, the draws are pure functions) / LRG_STAGE_ITER_CAP (an object's loop reached max_iters passes), tuples, arena words
 * used, objects stored.  visited and cur_mask of a listed room are cleared by the launch itself.
 * Limits: rooms below 2^30 points, 1 <= max_points <= LRG_STAGE_MAX_POINTS.  Refused with LRG_EINVAL - 100 .. - 103.
 *
 * lrg_stage_tuples: one workgroup per row of table [n_tuples, 8] = room, inlier count, neighbour count, offsets of the two lists in
 * `arena` (absolute), first output row of the inlier side, of the neighbour side, 0.  It takes numpy.median's float32 result of the
 * channels 0, 1 and 6 .. F-1 over the emitted inlier rows (:234-235), subtracts it from both sides in float32 (:236-240) and writes
 * points [rows, F] / remove [rows] and neighbor_points [rows, F] / add [rows].  Refused with LRG_EINVAL - 105 .. - 107. */
#define LRG_STAGE_MAX_POINTS 1024
#define LRG_STAGE_MAX_FEATURES 64
#define LRG_STAGE_OK 0
#define LRG_STAGE_OVERFLOW 1
#define LRG_STAGE_ITER_CAP 2
/* stage_data.py:104-231 */
int lrg_stage_teacher(const LrgRoom *rooms, const int32_t *room_list, int n_list, const int64_t *ws_off, uint8_t *cur_mask, int32_t *lists,
                      int32_t *arena, const int64_t *arena_off, const int32_t *arena_cap, int32_t *objects, int32_t *status, uint32_t rng_seed,
                      int max_points, int cluster_threshold, int max_steps, int max_iters, void *stream);
/* stage_data.py:233-240 */
int lrg_stage_tuples(const LrgRoom *rooms, const int32_t *arena, const int32_t *table, int n_tuples, int F, float *points, int32_t *remove,
                     float *neighbor_points, int32_t *add, void *stream);

/* ------------------------------------------------------------------------------------------------
 * ABI 23.  SemanticKITTI scans fused into scenes (stage_semantic_kitti.py), one sample (a stack of `interval` scans) per call,
 * one thread per point in every launch.  All arithmetic is float64 in plain chains of unfused products and sums, the IEEE division and rint.
 * A table is a linear-probe hash of packed voxel keys: keys [slots] and vals [slots] from the caller, slots a power of two of at least
 * max(64, 2 n) (lrg_kitti_table_slots (n); 0 for an n the calls refuse); every call fills its table itself.  A slot holds the smallest index
 * that inserted its key (CAS on the key, atomicMin on the value).  status [1] is cleared by every call and collects LRG_KITTI_ST_* bits: a
 * coordinate that is not finite, a voxel outside the 21-bit key window (less one cell either side, for the neighbour probes), a scan index out
 * of range, a full table.  With a bit set the outputs are not to be used.  Every result is a minimum, an integer sum or a minimum-index root,
 * so a call writes the same bytes every time.  Limits: n <= LRG_KITTI_MAX_POINTS.
 *
 * lrg_kitti_project: points [n, ld] float32 (x y z first) of n_scans scans back to back in (scan, index) order, scan_of [n] ascending,
 * labels [n] (object << 16 | class), pose [n_scans, 12] = the first three rows of Tr^-1 pose Tr of every scan, tr [16] and p2 [12] the
 * calibration's rows, images = the scans' RGB images in one buffer, scan s at img_off [s] with img_h [s] rows of img_w [s] pixels.
 * Writes xyz [n, 3] = ((r0 x + r1 y) + r2 z) + t; valid [n]: h = P2 (Tr [x y z 1]) in the same four-term chains, u = rint (h0 / h2),
 * v = rint (h1 / h2), valid when h2 > 0, 0 <= u < W and 0 <= v < H, compared as doubles; rgb [n, 3]: image [v, u] of a valid point; an
 * invalid point takes the colour of the smallest valid index of its voxel, rint (xyz / voxel_resolution), when that index belongs to a scan
 * not later than its own, else 0 0 0; keep [n] = colour not 0 0 0 and class < 250.  Refused with LRG_EINVAL - 110 .. - 112.
 *
 * lrg_kitti_first_in_voxel: rep [i] = the smallest index whose voxel rint (xyz / resolution) is that of point i.  Refused with
 * LRG_EINVAL - 113 .. - 115.
 *
 * lrg_kitti_components: for equalised points (one per voxel), every point with obj == 0 probes its 26 neighbour voxels and is joined to each
 * point found there whose cls equals its own (lrg_union.h; it `emits` an edge then).  Writes root [n] (the minimum index of the point's
 * component), and at every root size [root] (points of the component) and first_src [root] (its smallest emitting member; INT_MAX without
 * one); emits [n].  Refused with LRG_EINVAL - 116 .. - 118. */
#define LRG_KITTI_MAX_POINTS (1 << 28)
#define LRG_KITTI_ST_NONFINITE 1
#define LRG_KITTI_ST_WINDOW 2
#define LRG_KITTI_ST_SCAN 4
#define LRG_KITTI_ST_TABLE 8
int lrg_kitti_table_slots(int n);
/* stage_semantic_kitti.py:94-135 */
int lrg_kitti_project(const float *points, int ld, const int32_t *scan_of, const uint32_t *labels, int n, int n_scans, const double *pose,
                      const double *tr, const double *p2, const uint8_t *images, const int64_t *img_off, const int32_t *img_h,
                      const int32_t *img_w, double voxel_resolution, uint64_t *keys, int32_t *vals, int slots, double *xyz, uint8_t *rgb,
                      uint8_t *valid, uint8_t *keep, int32_t *status, void *stream);
/* stage_semantic_kitti.py:23-31, :144-154 */
int lrg_kitti_first_in_voxel(const double *xyz, int n, double resolution, uint64_t *keys, int32_t *vals, int slots, int32_t *rep,
                             int32_t *status, void *stream);
/* stage_semantic_kitti.py:167-183 */
int lrg_kitti_components(const double *xyz, const int32_t *obj, const int32_t *cls, int n, double resolution, uint64_t *keys, int32_t *vals,
                         int slots, int32_t *root, int32_t *size, int32_t *first_src, uint8_t *emits, int32_t *status, void *stream);

/* ------------------------------------------------------------------------------------------------
 * ABI 24.  Training batches for LrgNet assembled on the device (train_region_grow.py:156-175: every tuple of a batch padded /
 * subsampled to the network's point counts; the losses that consume them are learn_region_grow_util.py:165-186; DESIGN 3.20;
 * csrc/lrg_assemble.hip).  One side of one batch per call: rows [*, row_stride] float32 and labels [*] int32 are a side's flat buffers
 * (lrg_stage_tuples' points / remove or neighbor_points / add, or a staged file uploaded as it is), row_start [T] int64 and
 * row_count [T] int32 the first row and the number of rows of every kept tuple, order [B] the tuple ids of the batch.  Slot j < k of
 * instance b, with t = order[b] and N = row_count[t], is row row_start[t] + lrg_sample_position(j, N, k, purpose, 0, pass, epoch,
 * rng_seed, t) of csrc/lrg_rng.h (purposes TRAIN_INLIER 11, TRAIN_NEIGHBOR 12; pass 0 training, 1 validation): N >= k a subset without
 * replacement, N < k the N rows followed by draws with replacement, as the reference pads -- under the counter stream, a build
 * extension (the reference draws from one legacy stream), so a tuple's draws depend on (rng_seed, t, epoch, pass) alone.
 * Writes out_rows [B, k, F] (the F leading columns), out_labels [B, k] and positives [B] (the sum of the instance's gathered labels;
 * no atomics: the same bytes every time).  N >= 1 and t < T are the caller's contract.  Refused before any launch: LRG_EINVAL - 120 a
 * NULL pointer, - 121 B < 1, - 122 k outside 1 .. LRG_ASSEMBLE_MAX_POINTS, - 123 F < 1 (or above 65536), - 124 F > row_stride,
 * - 125 epoch, pass or purpose outside the counter's fields. */
#define LRG_ASSEMBLE_MAX_POINTS 4096
int lrg_train_assemble(const float *rows, int row_stride, const int32_t *labels, const int64_t *row_start, const int32_t *row_count,
                       const int32_t *order, int B, int k, int F, uint32_t rng_seed, int epoch, int pass, int purpose, float *out_rows,
                       int32_t *out_labels, int32_t *positives, void *stream);

/* ------------------------------------------------------------------------------------------------
 * ABI 25.  Growth trace and frames of animate_region_growing.py (csrc/lrg_trace.hip).  All three calls read the
 * grower's buffers and write the caller's; none changes a grow kernel's state.
 *
 * lrg_trace_snapshot: one snapshot of slot `slot` growing room `room` (greedy growing under the counter stream), enqueued behind
 * each lrg_grow_step_packed.  After a packed iteration an ACTIVE slot stands between evaluation and mask update, so a snapshot
 * starts the frame of the step just evaluated -- header (8 words: slot.seed, slot.step + 1 as animate_region_growing.py:374 counts,
 * room.next_cluster_id, then the counts of :398-401 over the raw points: inlier, neighbour, add, remove; word 7 becomes 1 once the
 * frame is complete) and a code byte per equalised point, bit 0 = previousMask (:365), bit 1 = the neighbour mask (:318-320) -- and
 * completes the frame before it: bit 2 = currentMask after the update (:366-373), which is the slot's mask while the slot is on the
 * same seed one step on, else the points visited since the frame began less the seeds of the zero-step 'noneighbor' regions logged
 * behind the finished one.  paint [stride] restates instance_color[currentMask] = instance_color_id[cluster_id] (:403) as
 * paint[after] = (next_cluster_id - 1) % 19 + 1 (the reference's 20-row table would raise at cluster 20; the wrap is ours); the frame's
 * copy goes to paints.  Frames live in rings of cap_frames rows: headers [cap_frames, 8], codes / paints [cap_frames, stride];
 * frame f is row f % cap_frames and `consumed` is the number of frames the host has taken.  state [8] (zeroed by the caller once):
 * [0] frames begun, [1] 1 while the last one awaits its `after`, [2] room.n_regions when it began, [3] error bits (1 a step without a
 * successor, 2 a list entry outside the room, 4 the ring is full, 8 not the room the buffers were sized for), [4] frames completed.
 * plan [8] and mark [stride] are scratch (zeroed once), vis_prev [stride] a copy of the visited flags, mult [stride] int32 the number of
 * raw points per equalised point (:123's unequalized_idx counted).  n = the room's points, stride >= n a multiple of 16; the byte
 * arrays and mult 16-byte aligned.  Every list entry is checked against n before it is used as an address. */
int lrg_trace_snapshot(const LrgSlot *slots, const LrgRoom *rooms, int slot, int room, int n, int stride, int cap_frames, int consumed,
                       int32_t *state, int32_t *plan, int32_t *headers, uint8_t *codes, uint8_t *paints, uint8_t *paint,
                       uint8_t *vis_prev, uint8_t *mark, const int32_t *mult, void *stream);

/* displayFun of animate_region_growing.py:165-182 (glPointSize squares of GL_POINTS under GL_DEPTH_TEST) once per camera instead of
 * once per frame: vis [H * W] receives per pixel the smallest key (bits(depth) << 32) | raw index of the points covering it, all ones
 * where there is none.  xyz [M, 3] float32 raw points; matrix_host: HOST pointer to the 16 floats, row-major, of projection x view
 * (gluPerspective x gluLookAt, :169,:255).  Per point in float32 without fused multiply-adds: clip_r = ((m[4r] x + m[4r+1] y) + m[4r+2] z)
 * + m[4r+3]; kept if w > 0 and -w <= x, y, z <= w; ndc = clip / w; xw = (ndc.x * 0.5 + 0.5) * W, yw likewise with H; depth = ndc.z * 0.5
 * + 0.5; the pixels [floor(xw) - h, floor(xw) + h] x [floor(yw) - h, floor(yw) + h], h = (point_size - 1) / 2, clipped to the window, image
 * row H - 1 - y (:394).  The result does not depend on the order of execution.  LRG_EINVAL - 1: point_size even or outside 1 .. 63. */
int lrg_render_visibility(const float *xyz, int M, const float *matrix_host, int W, int H, int point_size, unsigned long long *vis,
                          void *stream);

/* T palette-index frames out [T, H, W] uint8 through one visibility buffer (:387,:404 result_points[:,3:6] = colour[unequalized_idx]):
 * pixel = luts[frame_lut[t]][index[t * index_stride + unequalized_idx[vis & 0xffffffff]]], 0 where vis is all ones.  luts [n_luts, 256].
 * text (nullable) [T, 5, text_len] bytes: the five lines of :397-401 per frame (0 = nothing), drawn with value `white` from font
 * [font_count, 7] (glyphs of 5 x 7 bits for the characters font_first ..., bit 4 = leftmost) in cells of 6 x 8 font pixels, each
 * max(1, 40 H / 8000) screen pixels, at x = 10 H / 1000, y = (10 + 50 k) H / 1000 (integer division). */
int lrg_render_shade(const unsigned long long *vis, const int32_t *unequalized_idx, int M, int n, int W, int H, int T,
                     const uint8_t *index, long index_stride, const uint8_t *luts, int n_luts, const int32_t *frame_lut,
                     const uint8_t *text, int text_len, const uint8_t *font, int font_first, int font_count, int white, uint8_t *out,
                     void *stream);

/* ------------------------------------------------------------------------------------------------
 * ABI 26.  The ASCII vertex lines of savePLY / savePCD (learn_region_grow_util.py:33-73) encoded on the device, byte for byte what
 * Python's '%' operator gives (csrc/lrg_text.hip).  lrg_text_encode: n rows -- all rooms of a call back to back -- of
 * xyz [n, ld] float32 (x, y, z in the first three columns, ld >= 3) and rgb [n, 3] int32 become
 *   LRG_TEXT_PLY  "%f %f %f %d %d %d\n"
 *   LRG_TEXT_PCD  "%f %f %f %d\n" with (r << 16) | (g << 8) | b
 * in text, line i at byte line_off[i]; line_off [n + 1] int32, line_off[n] the total, so the body of the rows [a, b) is
 * text[line_off[a] : line_off[b]].  '%f' of a float32 is exact integer arithmetic: x 10^6 = (m 15625) 2^(e + 6) with m < 2^24, one
 * round-half-even on the bits shifted out, the sign printed for -0.0 and for negatives that round to zero.  A row is REFUSED -- a line
 * of zero bytes, counted in *status (int32 on the device, set by this call) -- if a coordinate is not finite or |x| >= 2^40, and
 * under LRG_TEXT_PCD if a colour is outside 0 .. 255; the caller writes such a room on the host.  With |x| < 2^40 a '%f' field has at
 * most 21 bytes and a '%d' field 11, so no line is longer than LRG_TEXT_MAX_LINE; the caller sizes text from that bound:
 * text_bytes >= n * LRG_TEXT_MAX_LINE, text 16-byte aligned (nothing is read back to size it: one synchronisation, the caller's, before
 * the download of line_off[n] bytes).  Stream-ordered: length pass, the exclusive scan of lrg_scan.hip over the lengths (int32, hence
 * n * LRG_TEXT_MAX_LINE < 2^31 per call), write pass; nothing is allocated and nothing synchronised.  workspace:
 * lrg_text_workspace_bytes(n) bytes, 16-byte aligned.  Refused before any launch: LRG_EINVAL - 130 a NULL pointer or a misaligned
 * text / workspace, - 131 n < 0 or n * LRG_TEXT_MAX_LINE >= 2^31, - 132 ld < 3, - 133 an unknown format, - 134 workspace_bytes or
 * text_bytes too small.  n == 0 sets line_off[0] = 0 and *status = 0. */
#define LRG_TEXT_MAX_LINE 102
#define LRG_TEXT_PLY 0
#define LRG_TEXT_PCD 1
size_t lrg_text_workspace_bytes(int n);
int lrg_text_encode(const float *xyz, int ld, const int32_t *rgb, int n, int format, void *workspace, size_t workspace_bytes,
                    int32_t *line_off, uint8_t *text, size_t text_bytes, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LRG_HIP_H */
