"""GPU: the beam search at the limits of what it accepts.

lrg_beam_advance alone (the queue step: selection, parent copies, stall test, commit, next seed, child set-up) on hand-made child results
at every group shape up to 16 x 4 = 64 slots, against tests/beam_rooms.py's NumPy model of it, every comparison exact; and whole searches
(BeamSearchGrower, scoring 'np') against oracle/beam_ref.py driven by the same GPU network, as tests/test_gpu_beam.py does, at the group
shapes 16 x 4, 8 x 8, 1 x 64 and 16 x 1, with unequal set sizes, streamed networks, lite / feature-size variants, rooms away from the
origin and rooms of one or two points.

Times on one MI355X, oracle included (nearly all of it is the oracle's one network call per child; the device's share is 0.01-0.14 s):
the 3 x 3 'net' case of test_beam_search_matches_oracle took 3.78 s in the same run, and here
  group shapes 16 x 4: 1.84 s (2732 oracle evaluations), 8 x 8: 2.20 s (3632), 1 x 64: 6.71 s (5632, and a second seed: the first had a
  near-tie draw), 16 x 1: 0.15 s;  unequal sets 0.70 and 0.90 s;  streamed nets 0.33 s each;  lite / feature size 0.20, 1.45 and 3.72 s;
  placements 1.33 s;  tiny rooms 0.05 s;  lrg_beam_advance alone at most 0.33 s a case.
1 x 64 is 1.8 times the present 3 x 3 case, under the three times at which the strips would have been shortened.
"""
import ctypes
import time

import numpy as np
import pytest

from conftest import seed_without_near_tie

import beam_rooms
import placement_rooms
from beam_ml_ref import small_room
from learn_region_grow_amd import _lib, synthetic
from oracle import beam_ref, rng_ref

pytestmark = pytest.mark.gpu
WEIGHT_KW = dict(seed=0, gain=2.0, bias_std=0.2, add_bias_shift=0.0, rmv_bias_shift=-3.0)
SAME_LOGITS_MARGIN = 5e-7

@pytest.fixture(scope='module')
def nets(cuda_device):
    """make(n_inlier, n_neighbor, F, lite, mode) -> LrgNetHIP, one per configuration for the module"""
    from learn_region_grow_amd.lrgnet import LrgNetHIP
    made = {}

    def make(ni=128, nn=128, F=13, lite=0, mode='fused'):
        key = (ni, nn, F, lite, mode)
        if key not in made:
            w = synthetic.make_synthetic_weights(feature_size=F, lite=lite, **WEIGHT_KW)
            made[key] = LrgNetHIP(1, 1, ni, nn, F, lite, device=cuda_device, mode=mode).load_weights(w)
        return made[key]
    return make


def gpu_net_fn(net):
    def fn(xi, xn):
        _, add, _, rmv, _ = net.run(xi, xn)
        return add, rmv
    return fn


# ------------------------------------------------------------------------------------------------------------------------------
# lrg_beam_advance alone
# ------------------------------------------------------------------------------------------------------------------------------
class Direct:
    """A BeamSearchGrower's device buffers with room 0 bound to group 0 and nothing to group 1; the loop's kernels never run."""

    def __init__(self, net, room, BW, SW, scoring):
        import torch
        from learn_region_grow_amd.beam import BeamSearchGrower
        self.torch, self.BW, self.SW, self.G, self.n = torch, BW, SW, BW * SW, len(room['points'])
        self.gr = gr = BeamSearchGrower(net, rooms_in_flight=2, beam_width=BW, search_width=SW, seed=0, policy='net', scoring=scoring, trace=True)
        gr.load_rooms([room])
        gr.reset_state()
        gr.bind_group(0, 0)
        gr.bind_group(1, -1)

    def advance(self, BW=None, SW=None):
        gr = self.gr
        rc = gr.lib.lrg_beam_advance(ctypes.c_void_p(gr.d_groups.data_ptr()), ctypes.c_void_p(gr.d_slots.data_ptr()),
                                     ctypes.c_void_p(gr.d_rooms.data_ptr()), gr.n_groups, self.BW if BW is None else BW,
                                     self.SW if SW is None else SW, ctypes.byref(gr.params), ctypes.c_void_p(gr.d_stats.data_ptr()), None)
        self.torch.cuda.synchronize(gr.dev)
        return rc

    def write_children(self, children):
        """The results the loop's kernels would have left in the slots of group 0"""
        gr, torch = self.gr, self.torch
        slots = gr._read_slots()
        cur = np.zeros((len(children), gr.cap), dtype=np.uint8)
        for c, ch in enumerate(children):
            sl = slots[c]
            sl.updated, sl.scan_cnt, sl.ml_score = ch['updated'], ch['size'], ch['score']
            for d in range(3):
                sl.scan_mn[d], sl.scan_mx[d] = ch['mn'][d], ch['mx'][d]
            cur[c, :self.n] = ch['mask']
        gr.d_slots.copy_(torch.from_numpy(np.frombuffer(bytes(slots), dtype=np.uint8).copy()).to(gr.dev))
        gr.d_cur[:len(children)].copy_(torch.from_numpy(cur).to(gr.dev))

    def group(self, g=0):
        raw = self.gr.d_groups.cpu().numpy().tobytes()
        return _lib.LrgBeamGroup.from_buffer_copy(raw, g * ctypes.sizeof(_lib.LrgBeamGroup))

    def check(self, model, want, where):
        """Everything lrg_beam_advance leaves behind against the model, exactly"""
        gr, n, G = self.gr, self.n, self.G
        B = self.group()
        assert (B.done, B.pending) == (int(model.done), int(not model.done)), where
        slots = gr._read_slots()
        cur = gr.d_cur.cpu().numpy()
        for c, w in enumerate(want):
            sl = slots[c]
            assert (sl.status, sl.room) == (w['status'], w['room']), '%s slot %d' % (where, c)
            if w['status'] != beam_rooms.ACTIVE:
                continue
            got = (sl.seed, sl.step, sl.restart, sl.count, sl.ml_score, list(sl.mn), list(sl.mx), sl.updated)
            assert got == (w['seed'], w['step'], w['restart'], w['count'], w['ml_score'], w['mn'], w['mx'], -1), '%s slot %d' % (where, c)
            assert cur[c, :n].tobytes() == w['cur'].tobytes(), '%s: mask of child %d (parent %d)' % (where, c, c // self.SW)
            assert not cur[c, n:].any()
        for sl in slots[G:2 * G]:          # the group without a room
            assert (sl.status, sl.room) == (beam_rooms.IDLE, -1), where
        if not model.done:
            assert (B.seed, B.level, B.stuck, B.steps, B.nq) == (model.seed, model.level, model.stuck, model.steps, len(model.Q)), where
            assert (list(B.seq_mn), list(B.seq_mx)) == (model.seq_mn, model.seq_mx), where
            parent = gr.d_parent.cpu().numpy()[0]
            for k, q in enumerate(model.Q):
                assert (B.q_count[k], B.q_score[k]) == (q['count'], q['score']), '%s queue entry %d' % (where, k)
                assert (list(B.q_mn[3 * k:3 * k + 3]), list(B.q_mx[3 * k:3 * k + 3])) == (q['mn'], q['mx']), '%s queue entry %d' % (where, k)
                if model.level > 0:
                    assert B.q_parent[k] == k
                    assert parent[k, :n].tobytes() == q['mask'].tobytes(), '%s: parent mask %d' % (where, k)
                else:
                    assert B.q_parent[k] == -1 and k == 0          # the seed-only mask has no buffer
        R = gr._read_rooms()[0]
        assert (R.n_regions, R.next_cluster_id, R.seed_cursor, R.done) == (len(model.region_log), model.next_cluster_id, model.seed_cursor,
                                                                           int(model.room_done)), where
        assert gr.d_visited.cpu().numpy()[:n].tobytes() == model.visited.tobytes(), where
        np.testing.assert_array_equal(gr.d_label.cpu().numpy()[:n], model.label, err_msg=where)
        np.testing.assert_array_equal(gr.d_rlog.cpu().numpy()[:len(model.region_log)].reshape(-1, 8),
                                      np.asarray(model.region_log, dtype=np.int32).reshape(-1, 8), err_msg=where)
        return B


def _box(model):
    return (model.seq_mn, model.seq_mx)


@pytest.fixture(scope='module')
def direct_room():
    return beam_rooms.strip_room([(8, 300), (8, 301)], room_id=44)          # 607 points: several commits leave seeds to take


@pytest.mark.parametrize('scoring', ['np', 'ml'])
@pytest.mark.parametrize('BW,SW', beam_rooms.GROUP_SHAPES)
def test_advance_alone(nets, direct_room, BW, SW, scoring):
    ml = scoring == 'ml'
    room = direct_room
    d = Direct(nets(), room, BW, SW, scoring)
    model = beam_rooms.GroupModel(room, 0, BW, SW, ml)
    rs = np.random.RandomState(100 * BW + SW + ml)
    assert d.advance() == 0
    want = model.advance()
    d.check(model, want, 'first seed')
    assert model.seed == room['order'][0] and sum(w['status'] == beam_rooms.ACTIVE for w in want) == SW
    widest, seen = 0, set()
    for step, pattern in enumerate(beam_rooms.advance_script(BW, SW, ml)):
        n_children = len(model.Q) * SW
        widest = max(widest, n_children)
        children = beam_rooms.child_results(pattern, n_children, BW, SW, d.n, _box(model), rs)
        d.write_children(children)
        assert d.advance() == 0
        want = model.advance(children)
        assert not model.done, 'the script used the room up'
        d.check(model, want, 'step %d (%s, %d children)' % (step, pattern, n_children))
        seen.add((pattern, n_children))
    # the script did what it is for
    assert widest == (BW * SW if SW > 1 else 1)          # (one child per parent never widens the queue)
    assert 'dry' in model.commits and 'stall' in model.commits
    assert any(r[4] for r in model.region_log) and any(not r[4] for r in model.region_log)
    assert any(any(x[1] == 0 for x in e) for _, _, e in model.trace) == ml      # an emptied mask among the best: under 'ml' only
    if ml:
        assert any(any(x[2] == -np.inf for x in e) for _, _, e in model.trace)
    d.gr.drain_trace()
    assert d.gr.room_trace[0] == model.trace
    assert int(d.gr.d_stats[0].item()) == len(model.region_log)


def test_advance_finishes_a_room(nets):
    """A two-point room: both seeds are committed from their seed-only heads (a dry queue at level 0), then the room is done, the done
    ring names the group's first slot and every slot is idle -- also at the calls after that."""
    room = beam_rooms.tiny_room(2, room_id=2)
    BW, SW = 16, 4
    d = Direct(nets(), room, BW, SW, 'np')
    model = beam_rooms.GroupModel(room, 0, BW, SW, False)
    rs = np.random.RandomState(1)
    assert d.advance() == 0
    d.check(model, model.advance(), 'first seed')
    for step in range(4):
        children = beam_rooms.child_results('none', len(model.Q) * SW, BW, SW, d.n, _box(model), rs) if not model.done else None
        if children:
            d.write_children(children)
        assert d.advance() == 0
        d.check(model, model.advance(children), 'step %d' % step)
    assert model.done and model.commits == ['dry', 'dry'] and [r[:3] for r in model.region_log] == [[1, SW, 1], [0, SW, 1]]
    st = d.gr.d_stats.cpu().numpy()
    assert (st[0], st[1], st[4]) == (2, 1, 0)


@pytest.mark.parametrize('BW,SW', [(17, 1), (16, 5), (0, 3), (3, 0)])
def test_group_shapes_refused(nets, direct_room, BW, SW):
    from learn_region_grow_amd.beam import BeamSearchGrower
    with pytest.raises(ValueError):
        BeamSearchGrower(nets(), rooms_in_flight=1, beam_width=BW, search_width=SW)
    d = Direct(nets(), direct_room, 2, 2, 'np')
    before = d.gr.d_groups.cpu().numpy().tobytes(), d.gr.d_slots.cpu().numpy().tobytes()
    assert d.advance(BW, SW) == _lib.LRG_EINVAL - 1
    assert (d.gr.d_groups.cpu().numpy().tobytes(), d.gr.d_slots.cpu().numpy().tobytes()) == before          # nothing was launched


# ------------------------------------------------------------------------------------------------------------------------------
# whole searches against the oracle
# ------------------------------------------------------------------------------------------------------------------------------
def _search(net, rooms, BW, SW, in_flight, trace=False, lite=0, seeds=range(21, 29)):
    """-> (seed, device results, oracle results, per room {(seed point, level): children evaluated}); asserts regions and labels equal"""
    from learn_region_grow_amd.beam import BeamSearchGrower
    t0 = time.time()
    evaluated = {}

    def oracle(seed):
        out = []
        for i, room in enumerate(rooms):
            count = evaluated[i] = {}

            def hook(rec, count=count):
                count[(rec['seed'], rec['level'])] = count.get((rec['seed'], rec['level']), 0) + 1
            out.append(beam_ref.beam_room(room['points'], room['obj_id'], room['order'], None, rng_ref.CounterStream(seed, room['room_id']),
                                          net_fn=gpu_net_fn(net), policy='net', beam_width=BW, search_width=SW, lite=lite,
                                          num_inlier=net.num_inlier_points, num_neighbor=net.num_neighbor_points, hook=hook))
        return out
    seed, wants = seed_without_near_tie(oracle, seeds, SAME_LOGITS_MARGIN)
    t1 = time.time()
    got = BeamSearchGrower(net, rooms_in_flight=in_flight, beam_width=BW, search_width=SW, seed=seed, policy='net', trace=trace).run(rooms)
    t2 = time.time()
    print('beam %d x %d, %d/%d sets, %s, %d rooms, %d in flight: seed %d, %d oracle evaluations, oracle %.2f s, device %.2f s' % (
        BW, SW, net.num_inlier_points, net.num_neighbor_points, net.mode, len(rooms), in_flight, seed, sum(w.total_steps for w in wants), t1 - t0, t2 - t1))
    for g, want in zip(got, wants):
        assert [(r['seed'], r['steps'], r['points'], r['labeled']) for r in g.regions] == \
               [(r['seed'], r['steps'], r['points'], r['labeled']) for r in want.regions]
        np.testing.assert_array_equal(g.cluster_label, want.cluster_label)
        np.testing.assert_array_equal(g.filled_label, want.filled_label)
    return seed, got, wants, evaluated


@pytest.mark.parametrize('BW,SW,in_flight', [(16, 4, 1), (8, 8, 3), (1, 64, 1), (16, 1, 1)])
def test_group_shapes(nets, BW, SW, in_flight):
    rooms = [beam_rooms.strip_room(), beam_rooms.ml_crop_room()]          # (regions of the strips end by a dry queue only; the crop's heads stall)
    _, got, wants, evaluated = _search(nets(), rooms, BW, SW, in_flight, trace=True)
    # the case proves something only if the queue fills and a level has every child of the group (one child per parent never widens it)
    reach = BW if SW > 1 else 1
    assert max(len(entries) for _, _, entries in got[0].beam_trace) == reach
    assert max(evaluated[0].values()) == reach * SW
    assert any(r['labeled'] for r in wants[0].regions) and any(not r['labeled'] for r in wants[0].regions)


@pytest.mark.parametrize('ni,nn', [(64, 128), (128, 64)])
def test_unequal_sets(nets, ni, nn):
    _search(nets(ni, nn), [beam_rooms.strip_room(), beam_rooms.ml_crop_room()], 4, 4, 1)


@pytest.mark.parametrize('mode', ['streamed', 'streamed-tiles'])
def test_streamed_nets(nets, mode):
    """lrg_beam_level without row lists and sample maps: logits for all rows of every set.  Each mode against the oracle driven by that
    same network (the modes' logits differ in their last bits)."""
    _search(nets(mode=mode), [beam_rooms.strip_room()], 3, 3, 1)


@pytest.mark.parametrize('lite,F', [(1, 13), (2, 12), (0, 6)])
def test_lite_and_feature_size(nets, lite, F):
    room = small_room(800 + F, 900, furniture=3, room_id=F)
    room['points'] = np.ascontiguousarray(room['points'][:, :F])
    _search(nets(512, 512, F, lite), [room], 3, 3, 1, lite=lite)


def test_placements(nets):
    """The strip room below zero, far out and at the corner of the voxel keys' window, two of them in flight together"""
    base = beam_rooms.strip_room()
    rooms = [dict(placement_rooms.place(base, placement_rooms.PLACEMENTS[name](base)), room_id=50 + k)
             for k, name in enumerate(('negative', 'far', 'window'))]
    _search(nets(), rooms, 4, 4, 2)


def test_tiny_rooms(nets):
    """Rooms of one and two points and a room without an object above the cluster threshold, in more groups than rooms"""
    rooms = [beam_rooms.tiny_room(1, 1), beam_rooms.tiny_room(2, 2), beam_rooms.below_threshold_room()]
    _, got, wants, _ = _search(nets(), rooms, 3, 3, 5)
    assert [len(g.regions) for g in got[:2]] == [1, 2]
    for g, room in zip(got, rooms):
        assert sum(r['points'] for r in g.regions) == len(room['points']) and not g.cluster_label.any() and not g.filled_label.any()
