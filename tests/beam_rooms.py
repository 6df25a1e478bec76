"""Rooms, hand-made child results and a NumPy model of the beam search's queue step: host helpers of tests/test_gpu_beam_shapes.py,
tests/test_gpu_beam_ml.py and tests/test_beam_rooms_host.py (test infrastructure; not collected by pytest).

Rooms.  A group of 16 x 4 children costs the oracle 64 network evaluations per level, so the rooms of the large groups are small:

  strip_room()   median_rooms.make([(8, 96), (8, 97)]): two strips eight voxels wide with a three-point fence each, 199 points.  Under the
                 Bernoulli policy a search from a strip's corner widens level by level, so queues fill to beam_width and levels reach
                 beam_width * search_width children; the fences and the leftovers give regions below the cluster threshold.
  ml_crop_room() the box around one piece of furniture of small_room(710, 1200, furniture=3), the order re-derived over the crop.  The
                 strips' constant channels saturate the confidences, so the bound the twin of --scoring ml keeps explodes there; the
                 furniture room keeps it near 1e-5 but is too long a search at full size.  Self-follow figures (the twin following its own
                 trace with oracle/lrgnet_ref.py as the network, seed 21; tests/test_beam_rooms_host.py asserts the limits):
                 ML_CROP_FIGURES below.
  tiny rooms     one point, two points, and a room whose every object is below the cluster threshold.

The queue step.  GroupModel restates lrg_beam_advance_kernel (csrc/lrg_beam.inl) for one group in the terms of the reference script:
Q = sorted(newQ, key=score, reverse=True)[:BEAM_WIDTH], emptied masks dropped afterwards, the stall test on the head, the commit, the next
seed.  child_results() makes the hand-made results of a level (PATTERNS) that a test writes into the slots in place of the loop's kernels.
"""
import numpy as np

import median_rooms
from oracle.grow_ref import voxelize

RES = 0.1
STRIPS = [(8, 96), (8, 97)]
LOG_WORDS = 8
IDLE, ACTIVE = 0, 1

# what a level's children report, by name; the first group under either scoring, the second under --scoring ml only
PATTERNS_NP = ('distinct', 'equal', 'exactly_bw', 'fewer', 'no_neighbours', 'stall', 'none')
PATTERNS_ML = ('ml_distinct', 'ml_equal', 'ml_minus_inf', 'ml_all_minus_inf', 'ml_empty_on_top', 'ml_only_empties')
GROUP_SHAPES = [(16, 4), (8, 8), (4, 16), (1, 64), (16, 1), (1, 1), (3, 3)]


def strip_room(strips=STRIPS, room_id=30, F=13):
    return median_rooms.make(strips, room_id=room_id, F=F)


def crop(room, lo, hi, room_id):
    """The points of `room` inside the box [lo, hi] (xyz), in their order; the seed order re-derived over the crop."""
    pts, order = room['points'], np.asarray(room['order'])
    inside = np.all((pts[:, :3] >= np.asarray(lo, np.float64)) & (pts[:, :3] <= np.asarray(hi, np.float64)), axis=1)
    idx = np.nonzero(inside)[0]
    new = np.full(len(pts), -1, dtype=np.int64)
    new[idx] = np.arange(len(idx))
    return dict(points=np.ascontiguousarray(pts[idx]), obj_id=np.asarray(room['obj_id'])[idx], order=new[order[inside[order]]].astype(np.int32),
                room_id=room_id)


# ml_crop_room under --scoring ml, the twin following its own trace with oracle/lrgnet_ref.py as the network:
# (beam, search, n_inlier, n_neighbor, seed) -> (evaluations, pairs compared, pairs undecided, worst relative bound)
ML_CROP_FIGURES = {
    (8, 4, 128, 128, 21): (1052, 1001, 17, 1.6e-5), (8, 4, 128, 128, 22): (1256, 1177, 16, 1.8e-5),
    (4, 4, 64, 128, 21): (768, 702, 13, 1.5e-5), (4, 4, 64, 128, 22): (604, 517, 0, 1.5e-5),
}
ML_CROP_OBJECT, ML_CROP_PAD = 7, 0.35


def ml_crop_room(room_id=36):
    """290 points of small_room(710, 1200, furniture=3): the box 0.35 m around its first piece of furniture in x and y, from the floor to
    0.35 m above the piece -- the piece (70 points), parts of the floor, of a wall and of the two other pieces."""
    from beam_ml_ref import small_room
    room = small_room(710, 1200, furniture=3, room_id=35)
    piece = room['points'][np.asarray(room['obj_id']) == ML_CROP_OBJECT, :3].astype(np.float64)
    lo, hi = piece.min(axis=0) - [ML_CROP_PAD, ML_CROP_PAD, 1.0], piece.max(axis=0) + ML_CROP_PAD
    return crop(room, lo, hi, room_id)


def tiny_room(n, room_id):
    """n points of a box room, seven apart in its list, seeds last point first (the rooms of test_tiny_rooms)."""
    from beam_ml_ref import small_room
    room = small_room(900 + n, 600)
    keep = np.arange(n) * 7
    return dict(points=np.ascontiguousarray(room['points'][keep]), obj_id=np.asarray(room['obj_id'])[keep], order=np.arange(n)[::-1].copy(),
                room_id=room_id)


def below_threshold_room(room_id=41, cluster_threshold=10):
    """Strips of 6 and 7 points with their fences of 3, three empty voxels apart: a region can take a strip and its fence, never more --
    at most 10 points, so nothing is labelled whatever the masks."""
    room = strip_room([(2, 6), (7, 7)], room_id=room_id)
    assert max(c + 3 for _, _, c in room['strips']) <= cluster_threshold
    return room


# ------------------------------------------------------------------------------------------------------------------------------
# the selection and the queue step
# ------------------------------------------------------------------------------------------------------------------------------
def select(updated, size, score, ml, beam_width):
    """test_beam_search.py:282 on plain lists: -> (best, kept).  The candidates are the children whose mask changed, in child order."""
    key = score if ml else size
    new_q = [c for c, u in enumerate(updated) if u == 1]
    best = sorted(new_q, key=lambda c: key[c], reverse=True)[:beam_width]
    return best, [c for c in best if size[c] > 0]


def child_results(pattern, n_children, BW, SW, n, box, rs):
    """Hand-made results of one level: a list of n_children dicts(updated, size, mn, mx, score, mask).  Every mask is a distinct random
    subset of the room's n points (its first point always in, so that only 'emptied' masks are empty), so a copy from the wrong child
    shows.  box = (mn, mx) of the sequence so far: the children's boxes reach past it, except under 'stall', where they stay inside."""
    nq = n_children // SW
    mn0, mx0 = np.asarray(box[0]), np.asarray(box[1])
    top = max(1, min(n - 2, 96))          # masks of at most 97 points: several commits leave a room of a few hundred points its seeds
    sizes = 2 + rs.permutation(top)[:n_children] if n_children <= top else 2 + rs.randint(0, top, n_children)
    updated = np.ones(n_children, dtype=np.int64)
    score = -rs.permutation(4 * n_children)[:n_children] / 8.0 - 0.125          # distinct, exact in float64
    emptied = []
    if pattern in ('equal', 'ml_equal'):
        sizes[:] = 30
        score[:] = -2.5
    elif pattern == 'exactly_bw':
        updated[:] = 0
        updated[rs.permutation(n_children)[:min(BW, n_children)]] = 1
    elif pattern == 'fewer':
        updated[:] = 0
        updated[rs.permutation(n_children)[:max(1, min(BW, n_children) - 1)]] = 1
    elif pattern == 'no_neighbours':          # the last parent found no neighbours (lrg_box_query stopped its children: updated stays -1)
        updated[(nq - 1) * SW:] = -1
        if nq == 1:
            updated[:] = -1
    elif pattern == 'none':
        updated[:] = rs.randint(0, 2, n_children) - 1          # 0 (unchanged) or -1
        updated[0] = 0
    elif pattern == 'ml_minus_inf':
        score[rs.permutation(n_children)[:max(1, n_children // 2)]] = -np.inf
    elif pattern == 'ml_all_minus_inf':
        score[:] = -np.inf
    elif pattern == 'ml_empty_on_top':          # an emptied mask with the best score: it takes a place, then is dropped
        emptied = [int(rs.randint(0, n_children))]
        score[emptied[0]] = 0.0
    elif pattern == 'ml_only_empties':          # the best beam_width are all emptied masks: the queue runs dry though children were updated
        emptied = list(range(n_children)) if n_children <= BW else sorted(rs.permutation(n_children)[:BW].tolist())
        score[emptied] = 0.0 + np.arange(len(emptied)) * 0.0
    out = []
    for c in range(n_children):
        mask = np.zeros(n, dtype=np.uint8)
        size = min(int(sizes[c]), n)
        if c in emptied:
            size = 0
        else:
            mask[0] = 1
            mask[1 + rs.permutation(n - 1)[:size - 1]] = 1
        if pattern == 'stall':
            mn, mx = mn0 + rs.randint(0, 2, 3), mx0 - rs.randint(0, 2, 3)
            mn, mx = np.minimum(mn, mx), np.maximum(mn, mx)
        else:
            mn, mx = mn0 - 1 - rs.randint(0, 3, 3), mx0 + 1 + rs.randint(0, 3, 3)
        out.append(dict(updated=int(updated[c]), size=size, mn=[int(v) for v in mn], mx=[int(v) for v in mx], score=float(score[c]), mask=mask))
    return out


class GroupModel:
    """One group of lrg_beam_advance, and its room, on the host.  advance(children) takes the results of the level just evaluated (None at
    the first call) and returns the next level's slots: a list of BW * SW dicts -- status, room and, for the active ones, seed, step,
    restart, count, ml_score, mn, mx, updated, cur."""

    def __init__(self, room, room_index, BW, SW, ml, cluster_threshold=10, resolution=RES):
        self.BW, self.SW, self.ml, self.threshold, self.room_index = BW, SW, bool(ml), cluster_threshold, room_index
        self.voxels = voxelize(room['points'][:, :3], resolution)
        self.order = np.asarray(room['order'])
        self.n = len(self.order)
        self.visited = np.zeros(self.n, dtype=np.uint8)
        self.label = np.zeros(self.n, dtype=np.int32)
        self.region_log, self.next_cluster_id, self.seed_cursor, self.room_done = [], 1, 0, False
        self.seed, self.level, self.stuck, self.steps, self.pending, self.done = -1, 0, 0, 0, False, False
        self.Q, self.trace, self.commits = [], [], []          # commits: 'dry' | 'stall' per region, for the tests' own bookkeeping

    def _commit(self, why):
        head = self.Q[0]
        labeled = head['count'] > self.threshold
        mask = head['mask'].astype(bool)
        self.visited[mask] = 1
        if labeled:
            self.label[mask] = self.next_cluster_id
            self.next_cluster_id += 1
        self.region_log.append([self.seed, self.steps, head['count'], 0, int(labeled), 0, -1, -1])
        self.commits.append(why)
        self.seed = -1

    def _idle(self):
        return [dict(status=IDLE, room=-1) for _ in range(self.BW * self.SW)]

    def advance(self, children=None):
        BW, SW = self.BW, self.SW
        if self.done:
            return self._idle()
        if self.pending:
            nq = len(self.Q)
            assert len(children) == nq * SW
            self.steps += SW * sum(children[q * SW]['updated'] >= 0 for q in range(nq))          # :274; a parent without neighbours ran nothing (:212)
            best, kept = select([c['updated'] for c in children], [c['size'] for c in children], [c['score'] for c in children], self.ml, BW)
            self.trace.append((self.seed, self.level, [(c, children[c]['size'], children[c]['score'] if self.ml else float(children[c]['size']))
                                                       for c in best]))
            if not kept:
                self._commit('dry')                                                               # :179
            else:
                self.Q = [dict(count=children[c]['size'], mask=children[c]['mask'].copy(), score=children[c]['score'] if self.ml else 0.0,
                               mn=list(children[c]['mn']), mx=list(children[c]['mx'])) for c in kept]
                self.level += 1
            self.pending = False
        while True:
            if self.seed < 0:
                pos = next((p for p in range(self.seed_cursor, self.n) if not self.visited[self.order[p]]), None)
                if pos is None:
                    self.seed_cursor, self.room_done, self.done = self.n, True, True
                    return self._idle()
                sd = int(self.order[pos])
                self.seed_cursor = pos + 1
                self.seed, self.level, self.stuck, self.steps = sd, 0, 0, 0
                only = np.zeros(self.n, dtype=np.uint8)
                only[sd] = 1
                v = [int(x) for x in self.voxels[sd]]
                self.Q = [dict(count=1, mask=only, score=0.0, mn=list(v), mx=list(v))]           # :164-174
                self.seq_mn, self.seq_mx = list(v), list(v)
            head = self.Q[0]
            grew = any(a < b for a, b in zip(head['mn'], self.seq_mn)) or any(a > b for a, b in zip(head['mx'], self.seq_mx))      # :188-198
            if not grew and self.stuck >= 1:
                self._commit('stall')
                continue
            self.stuck = 0 if grew else self.stuck + 1
            self.seq_mn = [min(a, b) for a, b in zip(self.seq_mn, head['mn'])]
            self.seq_mx = [max(a, b) for a, b in zip(self.seq_mx, head['mx'])]
            break
        out = []
        for c in range(BW * SW):
            if c < len(self.Q) * SW:
                q = self.Q[c // SW]
                out.append(dict(status=ACTIVE, room=self.room_index, seed=self.seed, step=self.level, restart=c, count=q['count'],
                                ml_score=q['score'], mn=q['mn'], mx=q['mx'], updated=-1, cur=q['mask']))
            else:
                out.append(dict(status=IDLE, room=-1))
        self.pending = True
        return out


def advance_script(BW, SW, ml):
    """The patterns of one direct test, level after level: the queue widens to beam_width first (all children updated), every pattern then
    meets the widest level it can; 'stall' twice commits by the stall rule, 'none' and 'ml_only_empties' by a dry queue."""
    widen = ['distinct'] * 3
    script = widen + ['equal', 'distinct', 'exactly_bw', 'distinct', 'distinct', 'fewer'] + widen + ['no_neighbours'] + widen + ['stall', 'stall'] + \
        widen + ['none', 'none'] + widen
    if ml:
        script = ['ml_distinct' if p == 'distinct' else p for p in script]
        for p in ('ml_equal', 'ml_minus_inf', 'ml_all_minus_inf', 'ml_empty_on_top', 'ml_only_empties'):
            script += [p] + ['ml_distinct'] * 3
        script += ['ml_empty_on_top', 'ml_empty_on_top', 'none']
    return script


def g64_cases(seed=3):
    """(name, ml, BW, SW, updated, size, score) of every pattern at the widest level of every group shape: the inputs of the selection,
    for the host table tool."""
    rs = np.random.RandomState(seed)
    out = []
    for BW, SW in GROUP_SHAPES:
        for ml, names in ((0, PATTERNS_NP), (1, PATTERNS_NP + PATTERNS_ML)):
            for p in names:
                nq = BW if SW > 1 else 1
                ch = child_results(p, nq * SW, BW, SW, 199, ([0, 0, 0], [5, 5, 0]), rs)
                out.append(('%s_%dx%d_%s' % (p, BW, SW, 'ml' if ml else 'np'), ml, BW, SW, [c['updated'] for c in ch], [c['size'] for c in ch],
                            [c['score'] if ml else float(c['size']) for c in ch]))
    return out
