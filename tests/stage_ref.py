"""Twin of the staging teacher (stage_data.py:104-231 of the reference), for tests/test_stage_host.py and tests/test_gpu_stage.py.

``stage_room_twin`` restates the reference's loop line by line; every random draw goes through one small object:

``LegacyDraws(rs)``            the reference's calls on one legacy RandomState, in the reference's order -- under it the twin must equal
                               ``learn_region_grow_amd.stage.stage_room``, which the reference's own output pins (tests/golden/stage_room150.npz);
``CounterDraws(seed, room)``   the counter stream of the device teacher (csrc/lrg_stage.hip), on oracle.rng_ref: every draw a pure function
                               of (object seed, pass, point), the mistake test in integers.
"""
import numpy as np

from oracle import rng_ref

STAGE_SEED, STAGE_PROB, STAGE_ADD, STAGE_RMV, STAGE_INLIER, STAGE_NEIGHBOR = 5, 6, 7, 8, 9, 10


class IterCap(RuntimeError):
    """An object's loop reached max_iters passes (the device reports LRG_STAGE_ITER_CAP at the same point)."""


class LegacyDraws:
    def __init__(self, rs):
        self.rs = rs

    def seed_order(self, n):
        return self.rs.choice(range(n), n, replace=False)                   # :107

    def begin_object(self, seed_id):
        self.p_add = self.rs.randint(2, 5) * 0.1                             # :128
        self.p_rmv = self.rs.randint(2, 5) * 0.1                             # :129

    def add_mistakes(self, idx, t):
        return self.rs.random_sample(len(idx)) < self.p_add                  # :158

    def remove_mistakes(self, idx, t):
        return self.rs.random_sample(len(idx)) < self.p_rmv                  # :169

    def subset(self, n, k, purpose, t):
        return self.rs.choice(n, k, replace=False)                           # :179, :189

    def emitted(self):
        self.p_add = max(self.p_add - 0.01, 0.0)                             # :198
        self.p_rmv = max(self.p_rmv - 0.01, 0.0)                             # :199


class CounterDraws:
    def __init__(self, seed, room_id):
        self.cs = rng_ref.CounterStream(seed, room_id)

    def _words(self, idx, purpose, ctx):
        """word(j, purpose, ctx) for every j of idx: Philox block j >> 2, lane j & 3 (CounterStream._raw at arbitrary slots)."""
        idx = np.asarray(idx, dtype=np.uint64)
        seed_point, restart, step = ctx
        w = rng_ref.philox4x32_10(idx >> np.uint64(2), np.uint64(step), np.uint64(seed_point),
                                  np.uint64((purpose & 0xFF) | ((restart & 0xFFFFFF) << 8)), self.cs.k0, self.cs.k1)
        w = np.stack(w, axis=1)
        return [int(x) for x in w[np.arange(len(idx)), (idx & np.uint64(3)).astype(np.int64)]]

    def seed_order(self, n):
        if n == 1:
            return np.zeros(1, dtype=np.int64)
        keys = self.cs._raw(4, rng_ref.PURPOSE_PERMKEY | STAGE_SEED, (0, 0, 0))
        return rng_ref.feistel_permute(np.arange(n), n, keys)

    def begin_object(self, seed_id):
        self.s = int(seed_id)
        w = self._words([0, 1], STAGE_PROB, (self.s, 0, 0))
        self.p_add = 10 * (2 + ((w[0] * 3) >> 32))                           # hundredths
        self.p_rmv = 10 * (2 + ((w[1] * 3) >> 32))

    def add_mistakes(self, idx, t):
        return np.array([(w >> 8) * 100 < (self.p_add << 24) for w in self._words(idx, STAGE_ADD, (self.s, 0, t))], dtype=bool)

    def remove_mistakes(self, idx, t):
        return np.array([(w >> 8) * 100 < (self.p_rmv << 24) for w in self._words(idx, STAGE_RMV, (self.s, 0, t))], dtype=bool)

    def subset(self, n, k, purpose, t):
        keys = self.cs._raw(4, rng_ref.PURPOSE_PERMKEY | purpose, (self.s, 0, t))
        return rng_ref.feistel_permute(np.arange(k), n, keys)

    def emitted(self):
        self.p_add = max(self.p_add - 1, 0)
        self.p_rmv = max(self.p_rmv - 1, 0)


def stage_room_twin(points, obj_id, draws, resolution=0.1, cluster_threshold=10, max_points=1024, max_steps=500, max_iters=None, stats=None):
    """The dict of lists stage.stage_room returns (rows not yet centred).  `stats` (a dict) collects what the coverage checks ask:
    'passes' per object, 'sub_in' / 'sub_nb' (subsampled sides), 'stored', 'completed', 'small_dropped' (objects of at most
    cluster_threshold points that end without a steps entry), 'max_in' (largest emitted inlier side)."""
    points = np.asarray(points, dtype=np.float32)
    obj_id = np.asarray(obj_id)
    if max_iters is None:
        max_iters = 2 * max_steps + 64
    if stats is None:
        stats = {}
    stats.update(passes=[], sub_in=0, sub_nb=0, stored=0, completed=0, small_dropped=0, max_in=0)
    N = len(points)
    point_voxels = np.round(points[:, :3] / resolution).astype(int)                                     # :104
    visited = np.zeros(N, dtype=bool)                                                                   # :105
    out = dict(points=[], remove=[], neighbor_points=[], add=[], steps=[], complete=[])
    for seed_id in draws.seed_order(N):                                                                 # :107
        seed_id = int(seed_id)
        if visited[seed_id]:                                                                            # :109
            continue
        target_id = obj_id[seed_id]                                                                     # :111
        gt_mask = obj_id == target_id                                                                   # :113
        currentMask = np.zeros(N, dtype=bool)                                                           # :122
        currentMask[seed_id] = True
        minDims = point_voxels[seed_id].copy()                                                          # :124
        maxDims = point_voxels[seed_id].copy()
        steps = 0
        stuck = False
        draws.begin_object(seed_id)                                                                     # :128-129
        t = 0
        while True:                                                                                     # :138
            if t >= max_iters:
                raise IterCap('object seeded at %d: %d passes' % (seed_id, t))
            cur_idx = [i for i in np.nonzero(currentMask)[0]]                                           # :141, in point-index order
            inbox = np.logical_and(np.all(point_voxels >= minDims - 1, axis=1), np.all(point_voxels <= maxDims + 1, axis=1))   # :146
            cand_idx = [i for i in np.nonzero(inbox)[0] if not currentMask[i] and not visited[i]]      # :147-148
            expandClass = [bool(obj_id[i] == target_id) for i in cand_idx]                             # :152
            if stuck:                                                                                   # :154
                expandID = [i for i, c in zip(cand_idx, expandClass) if c]
            else:
                mistake = draws.add_mistakes(cand_idx, t)                                               # :158
                expandID = [i for i, c, m in zip(cand_idx, expandClass, mistake) if c != bool(m)]
            rejectClass = [bool(obj_id[i] != target_id) for i in cur_idx]                              # :163
            if stuck:
                rejectID = [i for i, c in zip(cur_idx, rejectClass) if c]
            else:
                mistake = draws.remove_mistakes(cur_idx, t)                                             # :169
                rejectID = [i for i, c, m in zip(cur_idx, rejectClass, mistake) if c != bool(m)]
            if len(cand_idx) > 0:                                                                       # :173
                if len(cur_idx) <= max_points:
                    rows = list(cur_idx)
                else:
                    subset = draws.subset(len(cur_idx), max_points, STAGE_INLIER, t)                    # :179
                    rows = [cur_idx[int(j)] for j in subset]
                    rejectClass = [rejectClass[int(j)] for j in subset]                                 # :182
                    stats['sub_in'] += 1
                out['points'].append(points[rows].copy())
                out['remove'].append(np.array(rejectClass, dtype=np.int32))
                stats['max_in'] = max(stats['max_in'], len(rows))
                if len(cand_idx) <= max_points:
                    rows = list(cand_idx)
                else:
                    subset = draws.subset(len(cand_idx), max_points, STAGE_NEIGHBOR, t)                 # :189
                    rows = [cand_idx[int(j)] for j in subset]
                    expandClass = [expandClass[int(j)] for j in subset]                                 # :192
                    stats['sub_nb'] += 1
                out['neighbor_points'].append(points[rows].copy())
                out['add'].append(np.array(expandClass, dtype=np.int32))
                inter = sum(1 for i in cur_idx if gt_mask[i])
                union = len(cur_idx) + int(gt_mask.sum()) - inter
                out['complete'].append(1.0 * inter / union)                                             # :194
                steps += 1
                draws.emitted()                                                                         # :198-199
            t += 1
            if np.all(currentMask == gt_mask):                                                          # :201
                visited[currentMask] = True
                out['steps'].append(steps)
                stats['stored'] += 1
                stats['completed'] += 1
                break
            if steps < max_steps and (any(expandClass) or any(rejectClass)):                            # :209
                for i in expandID:                                                                      # :212
                    currentMask[i] = True
                if len(rejectID) < len(cur_idx):                                                        # :213
                    for i in rejectID:
                        currentMask[i] = False
                nextMin = point_voxels[currentMask].min(axis=0)                                         # :215
                nextMax = point_voxels[currentMask].max(axis=0)
                if not np.any(nextMin < minDims) and not np.any(nextMax > maxDims):                     # :217
                    stuck = True
                minDims, maxDims = nextMin, nextMax
            else:                                                                                       # :224
                if np.sum(currentMask) > cluster_threshold:
                    visited[currentMask] = True
                    out['steps'].append(steps)
                    stats['stored'] += 1
                elif int(gt_mask.sum()) <= 10:
                    stats['small_dropped'] += 1
                break
        stats['passes'].append(t)
    return out


def center(staged):
    """stage_data.py:233-240 on a copy: what the device writes."""
    from learn_region_grow_amd import stage
    cp = dict(staged)
    cp['points'] = [p.copy() for p in staged['points']]
    cp['neighbor_points'] = [p.copy() for p in staged['neighbor_points']]
    return stage.center_tuples(cp)


# ---- the rooms of tests/test_gpu_stage.py, and their twin results, built once per session ----
RNG_SEED = 0
ROOM_IDS = (3, 7, 8, 20, 21)
_cache = {}


def prepared_room(n_equalized, seed):
    """(points [n,13] float32, obj_id [n]) of synthetic.area5_shaped_room, preprocessed on the host."""
    key = ('room', n_equalized, seed)
    if key not in _cache:
        from learn_region_grow_amd import preprocess, synthetic
        raw = synthetic.area5_shaped_room(n_equalized, seed=seed).astype(np.float32)
        p = preprocess.preprocess_room(raw[:, :6], raw[:, 6].astype(int), raw[:, 7].astype(int))
        _cache[key] = (p['points'], np.asarray(p['obj_id']))
    return _cache[key]


def gpu_rooms():
    """The five rooms of one launch: the 1500-point room, one point, 63 scattered points, the points of that room's largest object alone (a room
    that is all one object), the 6000-point room."""
    if 'rooms' not in _cache:
        a, e = prepared_room(1500, 1), prepared_room(6000, 2)
        ids, counts = np.unique(a[1], return_counts=True)
        one = a[1] == ids[np.argmax(counts)]
        rooms = [a, (a[0][:1], a[1][:1]), (a[0][::30][:63], a[1][::30][:63]), (a[0][one], a[1][one]), e]
        _cache['rooms'] = [dict(points=np.ascontiguousarray(p), obj_id=np.ascontiguousarray(o), room_id=rid) for (p, o), rid in zip(rooms, ROOM_IDS)]
    return _cache['rooms']


def twin(room_index, max_points=1024, seed=RNG_SEED):
    """(staged dict, rows not centred; stats) of room `room_index` of gpu_rooms() under CounterDraws(seed, its room id)."""
    key = ('twin', room_index, max_points, seed)
    if key not in _cache:
        room, stats = gpu_rooms()[room_index], {}
        _cache[key] = (stage_room_twin(room['points'], room['obj_id'], CounterDraws(seed, room['room_id']), max_points=max_points, stats=stats), stats)
    return _cache[key]
