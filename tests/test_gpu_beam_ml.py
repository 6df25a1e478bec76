"""GPU: the beam search under --scoring ml.  The score kernel alone (lrg_beam_ml_score on hand-made buffers) against the twin's
term sums within the twin's bound; whole searches (BeamSearchGrower(scoring='ml', trace=True)) FOLLOWED level by level by the twin
(tests/beam_ml_ref.py): candidate scores are often equal or ulps apart and the device's expf / logf are not NumPy's, so the twin checks
every choice the device made against its own scores and bounds, adopts the device's queue where it cannot tell, and the labels must
then agree exactly; 'np' with the trace on; the command line."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import seed_without_near_tie

import beam_ml_ref
from beam_ml_ref import small_room
from learn_region_grow_amd import _lib, checkpoint, metrics, synthetic
from learn_region_grow_amd import io as lio
from oracle import lrgnet_ref, metrics_ref, preprocess_ref, rng_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WEIGHT_KW = dict(seed=0, gain=2.0, bias_std=0.2, add_bias_shift=0.0, rmv_bias_shift=-3.0)
SAME_LOGITS_MARGIN = 5e-7
UNDECIDED_CAP = 0.10


@pytest.fixture(scope='module')
def net(cuda_device):
    from learn_region_grow_amd.lrgnet import LrgNetHIP
    return LrgNetHIP(1, 1, 512, 512, 13, 0, device=cuda_device).load_weights(synthetic.make_synthetic_weights(**WEIGHT_KW))


def gpu_net_fn(net):
    def fn(xi, xn):
        _, add, _, rmv, _ = net.run(xi, xn)
        return add, rmv
    return fn


@pytest.fixture(scope='module')
def rooms():
    return [small_room(710, 1200, furniture=3, room_id=35), small_room(300, 1500, furniture=4, room_id=13)]


# ------------------------------------------------------------------------------------------------------------------------------
# the kernel alone
# ------------------------------------------------------------------------------------------------------------------------------
RNG_SEED, ROOM_ID, RES = 77, 9, 0.1
SLOT_KINDS = ('full', 'padded', 'shared_voxel', 'saturated', 'saturated_minus_inf', 'idle', 'outside_fired', 'outside_not_fired')
OUTSIDE_X = 1.1e5      # metres: voxel 1 100 000 at 0.1 m, past the 2^20 that a voxel key holds (lrg_pack_voxel gives LRG_HASH_EMPTY)


def _hand_made(Ni, Nn, policy, data_seed, streamed=False):
    """Eight slots of hand-made step buffers (F = 13; Ni inlier rows, Nn neighbour rows) and what the twin makes of them.  -> dict of host
    arrays, per-slot expectations; None if a draw sits within 1e-5 of its confidence (the caller walks the data seeds).
    streamed: the buffers of a network that writes logits for ALL rows of a set (LrgStepBuffers.rows_in / rows_nb NULL): the 'padded' slot
    then carries logits of its own in every row, and a copy's term comes from ITS row's logits, not from the row it was copied from."""
    F, S = 13, len(SLOT_KINDS)
    rs = np.random.RandomState(data_seed)
    stream = rng_ref.CounterStream(RNG_SEED, ROOM_ID)
    h = dict(center=np.zeros((S, 16), np.float32), inlier=np.zeros((S, Ni, F), np.float32), neighbor=np.zeros((S, Nn, F), np.float32),
             add_logits=np.zeros((S, Nn, 2), np.float32), rmv_logits=np.zeros((S, Ni, 2), np.float32),
             gt_add=(rs.uniform(size=(S, Nn)) < 0.3).astype(np.int32), gt_remove=(rs.uniform(size=(S, Ni)) < 0.2).astype(np.int32),
             sample_in=np.tile(np.arange(Ni, dtype=np.int32), (S, 1)), sample_nb=np.tile(np.arange(Nn, dtype=np.int32), (S, 1)))
    slots, want = [], []
    for s, kind in enumerate(SLOT_KINDS):
        seed_pt, ordinal, level = 100 + 7 * s, s % 4, 1 + s
        parent = -0.75 - 0.5 * s                                   # a non-zero parent score in every slot
        nc, ne = 4 * Ni, 4 * Nn                                    # more points than rows: nothing padded
        h['center'][s, :2] = rs.randn(2) * 0.3
        for N, rows in ((Nn, h['neighbor']), (Ni, h['inlier'])):
            rows[s] = rs.randn(N, F) * 0.5
            # one point per voxel, as in an equalised room: rows on a grid of 0.2 with a jitter of 0.03 are >= 0.14 apart, more than a
            # voxel (0.1), so two rows share a voxel only where that is planted below
            rows[s, :, 0] = (np.arange(N) % 32) * 0.2 + rs.uniform(-0.03, 0.03, N)
            rows[s, :, 1] = (np.arange(N) // 32) * 0.2 + rs.uniform(-0.03, 0.03, N)
            rows[s, :, 2] = rs.uniform(-0.2, 0.2, N)
        h['add_logits'][s] = rs.randn(Nn, 2) * 1.5
        h['rmv_logits'][s] = rs.randn(Ni, 2) * 1.5
        u_add = stream.uniform(Nn, rng_ref.PURPOSE_ADD, (seed_pt, ordinal, level))
        u_rmv = stream.uniform(Ni, rng_ref.PURPOSE_RMV, (seed_pt, ordinal, level))
        if kind == 'padded':
            ne, nc = 5, 3                                          # rows 5.. / 3.. are copies; logits exist for the leading rows only
            for n_src, N, smp, rows, lg in ((ne, Nn, h['sample_nb'], h['neighbor'], h['add_logits']),
                                            (nc, Ni, h['sample_in'], h['inlier'], h['rmv_logits'])):
                smp[s, n_src:] = rs.randint(0, n_src, N - n_src)
                rows[s] = rows[s][smp[s]]
                if not streamed:
                    lg[s, n_src:] = 77.0 * np.array([1.0, -1.0])   # never written by the network: reading them gives conf 0 everywhere
        if kind.startswith('outside'):                             # the last row of each side lies outside the voxel keys' window, alone in
            fired = kind == 'outside_fired'                        # its voxel: it counts as fired if and only if its own draw fired
            for N, rows, lg, u, gt in ((Nn, h['neighbor'], h['add_logits'], u_add, h['gt_add']), (Ni, h['inlier'], h['rmv_logits'], u_rmv, h['gt_remove'])):
                rows[s, N - 1, 0] = OUTSIDE_X
                c = 0.5 * (1.0 + float(u[N - 1])) if fired else min(0.4, 0.5 * float(u[N - 1]) + 1e-3)      # above 0.5 and its draw / below both
                lg[s, N - 1] = (0.0, np.log(c / (1 - c)))
                gt[s, N - 1] = int(fired)
                if policy == 0 and (u[N - 1] >= 0.999 if fired else u[N - 1] < 0.01):
                    return None
        if kind == 'shared_voxel':
            for rows, lg, u, gt in ((h['neighbor'], h['add_logits'], u_add, h['gt_add']), (h['inlier'], h['rmv_logits'], u_rmv, h['gt_remove'])):
                rows[s, 1, :3] = rows[s, 0, :3]                    # two rows in one voxel: row 0 fires, row 1 does not
                lg[s, 0] = (0.0, 3.0)                              # conf 0.95: fires under the threshold; under the draws unless u >= 0.95
                c1 = min(0.4, 0.5 * float(u[1]) + 1e-3)            # conf below 0.5 and below its draw
                lg[s, 1] = (0.0, np.log(c1 / (1 - c1)))
                gt[s, 0], gt[s, 1] = 1, 0
                if policy == 0 and (u[0] >= 0.9 or u[1] < 0.01):
                    return None
        if kind.startswith('saturated'):
            for lg in (h['add_logits'], h['rmv_logits']):
                up = rs.uniform(size=lg.shape[1]) < 0.5
                lg[s, :, 0], lg[s, :, 1] = np.where(up, -100.0, 100.0), np.where(up, 100.0, -100.0)      # differences of +200 and -200
            h['gt_add'][s] = h['add_logits'][s, :, 1] > 0          # (policy 2 fires where conf = 1, as the other policies do)
            h['gt_remove'][s] = h['rmv_logits'][s, :, 1] > 0
            if kind == 'saturated_minus_inf':                      # a row of conf 0 in the voxel of a fired row: log(0)
                h['add_logits'][s, 0], h['add_logits'][s, 1] = (-100.0, 100.0), (100.0, -100.0)
                h['gt_add'][s, 0], h['gt_add'][s, 1] = 1, 0
                h['neighbor'][s, 1, :3] = h['neighbor'][s, 0, :3]
        sl = _lib.LrgSlot()
        sl.room, sl.status = 0, (_lib.LRG_IDLE if kind == 'idle' else _lib.LRG_ACTIVE)
        sl.seed, sl.restart, sl.step, sl.nc, sl.ne, sl.updated, sl.ml_score = seed_pt, ordinal, level, nc, ne, -1, parent
        slots.append(sl)
        # ---- the twin ----
        lo_nb = h['sample_nb'][s] if ne < Nn and not streamed else np.arange(Nn)
        lo_in = h['sample_in'][s] if nc < Ni and not streamed else np.arange(Ni)
        add_conf = lrgnet_ref.confidence(h['add_logits'][s][lo_nb])
        rmv_conf = lrgnet_ref.confidence(h['rmv_logits'][s][lo_in])
        if policy == 0:
            add_mask, rmv_mask = u_add < add_conf, u_rmv < rmv_conf
            margin = min(float(np.abs(u_add.astype(np.float64) - add_conf).min()), float(np.abs(u_rmv.astype(np.float64) - rmv_conf).min()))
            if margin < 1e-5 and not kind.startswith('saturated'):
                return None
        elif policy == 1:
            add_mask, rmv_mask = add_conf > 0.5, rmv_conf > 0.5
            if float(np.abs(np.concatenate([add_conf, rmv_conf]) - 0.5).min()) < 1e-5:
                return None
        else:
            add_mask, rmv_mask = h['gt_add'][s] != 0, h['gt_remove'][s] != 0
        center = np.zeros(F, np.float32)
        center[:2] = h['center'][s, :2]
        sides = beam_ml_ref.child_sides(h['neighbor'][s], h['inlier'][s], add_conf, rmv_conf, add_mask, rmv_mask, center, RES, Nn)
        score, err = beam_ml_ref.child_score(parent, 0.0, sides)
        want.append(dict(kind=kind, parent=parent, score=score, err=err, sides=sides, add_mask=add_mask, rmv_mask=rmv_mask))
    return dict(h=h, slots=slots, want=want)


def _run_score_kernel(lib, dev, made, Ni, Nn, policy, streamed=False):
    import torch
    S = len(made['slots'])
    d = {k: torch.from_numpy(v).to(dev) for k, v in made['h'].items()}
    room = _lib.LrgRoom()
    room.room_id = ROOM_ID
    d_rooms = torch.from_numpy(np.frombuffer(bytes(room), dtype=np.uint8).copy()).to(dev)
    d_slots = torch.from_numpy(np.frombuffer(b''.join(bytes(s) for s in made['slots']), dtype=np.uint8).copy()).to(dev)
    dummy = torch.zeros(16, dtype=torch.int32, device=dev)      # rows_in / rows_nb set: the sample maps are in force
    p = _lib.LrgGrowParams()
    p.resolution, p.feature_size, p.n_inlier, p.n_neighbor, p.cluster_threshold = RES, 13, Ni, Nn, 10
    p.restarts, p.group_size, p.rng_seed, p.policy, p.scoring = 1, 1, RNG_SEED, policy, 1
    b = _lib.LrgStepBuffers()
    for k in ('center', 'sample_in', 'sample_nb', 'inlier', 'neighbor', 'gt_remove', 'gt_add', 'add_logits', 'rmv_logits'):
        setattr(b, k, d[k].data_ptr())
    if not streamed:
        b.rows_in = b.rows_nb = dummy.data_ptr()
    _lib.check(lib.lrg_beam_ml_score(ctypes.c_void_p(d_slots.data_ptr()), ctypes.c_void_p(d_rooms.data_ptr()), S, ctypes.byref(p),
                                     ctypes.byref(b), None), 'lrg_beam_ml_score')
    torch.cuda.synchronize(dev)
    raw = d_slots.cpu().numpy().tobytes()
    sz = ctypes.sizeof(_lib.LrgSlot)
    return [_lib.LrgSlot.from_buffer_copy(raw, k * sz) for k in range(S)]


def _score_kernel_alone(lib, cuda_device, Ni, Nn, policy, streamed=False):
    made = None
    for data_seed in range(5, 25):
        made = _hand_made(Ni, Nn, policy, data_seed, streamed)
        if made is not None:
            break
    assert made is not None, 'every data seed tried has a draw within 1e-5 of its confidence'
    got = _run_score_kernel(lib, cuda_device, made, Ni, Nn, policy, streamed)
    again = _run_score_kernel(lib, cuda_device, made, Ni, Nn, policy, streamed)
    for sl, sl2, w in zip(got, again, made['want']):
        dev = sl.ml_score
        print('sets %d/%d policy %d %-20s device %.17g twin %.17g |diff| %.3g bound %.3g' % (
            Ni, Nn, policy, w['kind'], dev, w['score'], abs(dev - w['score']) if np.isfinite(w['score']) else 0.0, w['err']))
        assert np.float64(dev).tobytes() == np.float64(sl2.ml_score).tobytes(), w['kind']       # the same bits every run
        assert sl.step == sl2.step and sl.updated == -1                                         # (the kernel moves nothing else on)
        if w['kind'] == 'idle':
            assert dev == w['parent']                                                           # left alone
        elif w['kind'] == 'saturated':
            assert w['score'] == w['parent'] and dev == w['parent']                             # conf exactly 1 or 0: every term is 0
        elif w['kind'] == 'saturated_minus_inf':
            assert w['score'] == -np.inf and dev == -np.inf
        else:
            assert np.isfinite(w['score']) and np.isfinite(w['err']) and w['err'] < 1e-4 * abs(w['score'])
            assert abs(dev - w['score']) <= w['err'], w['kind']
            assert dev != w['parent']
    by = {w['kind']: w for w in made['want']}
    assert by['shared_voxel']['add_mask'][0] and not by['shared_voxel']['add_mask'][1]          # one of the two draws fired ...
    lg = made['h']['add_logits'][2, 1]
    c1 = lrgnet_ref.confidence(lg[None])[0]
    assert by['shared_voxel']['sides']['add_terms'][1] == np.log(c1) / np.float32(Nn)            # ... and its copy counts as fired
    for kind, fired in (('outside_fired', True), ('outside_not_fired', False)):                 # the rows outside the window: their own draws
        assert by[kind]['add_mask'][Nn - 1] == fired and by[kind]['rmv_mask'][Ni - 1] == fired
        k = SLOT_KINDS.index(kind)
        for lg, terms, N in ((made['h']['add_logits'], 'add_terms', Nn), (made['h']['rmv_logits'], 'rmv_terms', Ni)):
            c = lrgnet_ref.confidence(lg[k, N - 1][None])[0]
            assert by[kind]['sides'][terms][N - 1] == np.log(c if fired else np.float32(1.0) - c) / np.float32(Nn)
    if streamed:                                                                                # the copies' own logits decide, and they differ
        k = SLOT_KINDS.index('padded')
        smp, lg = made['h']['sample_nb'][k], made['h']['add_logits'][k]
        assert (smp[5:] < 5).all() and not np.array_equal(lg[smp], lg)


@pytest.mark.parametrize('N', [512, 64])
@pytest.mark.parametrize('policy', [0, 1, 2])
def test_score_kernel_alone(hip_lib, cuda_device, N, policy):
    _score_kernel_alone(hip_lib, cuda_device, N, N, policy)


@pytest.mark.parametrize('Ni,Nn', [(1024, 1024), (256, 1024), (1024, 64)])
@pytest.mark.parametrize('policy', [0, 1, 2])
def test_score_kernel_set_sizes(hip_lib, cuda_device, Ni, Nn, policy):
    """Two rows per thread and a full table at 1024; sides of unequal size: the remove side's rows start at slot * n_inlier and both sides
    divide by n_neighbor."""
    _score_kernel_alone(hip_lib, cuda_device, Ni, Nn, policy)


@pytest.mark.parametrize('Ni,Nn', [(512, 512), (1024, 1024), (256, 1024), (1024, 64)])
@pytest.mark.parametrize('policy', [0, 1, 2])
def test_score_kernel_streamed_form(hip_lib, cuda_device, Ni, Nn, policy):
    """rows_in / rows_nb NULL (a streamed network: logits for all rows), with fewer points than rows in one slot: row j's own logits"""
    _score_kernel_alone(hip_lib, cuda_device, Ni, Nn, policy, streamed=True)


# ------------------------------------------------------------------------------------------------------------------------------
# whole searches, followed level by level
# ------------------------------------------------------------------------------------------------------------------------------
def _twin(net, room, seed, beam, search, scoring, follow=None):
    return beam_ml_ref.beam_room(room['points'], room['obj_id'], room['order'], None, rng_ref.CounterStream(seed, room['room_id']),
                                 net_fn=gpu_net_fn(net), policy='net', beam_width=beam, search_width=search, scoring=scoring, follow=follow,
                                 num_inlier=net.num_inlier_points, num_neighbor=net.num_neighbor_points)


def _regions(res):
    return [(r['seed'], r['steps'], r['points'], r['labeled']) for r in res.regions]


@pytest.mark.parametrize('beam,search,in_flight', [(2, 2, 2), (3, 3, 1)])
def test_ml_search_followed_level_by_level(net, rooms, beam, search, in_flight):
    _followed_search(net, rooms, beam, search, in_flight)


@pytest.mark.parametrize('beam,search,ni,nn', [(8, 4, 128, 128), (4, 4, 64, 128)])
def test_ml_search_above_3x3(cuda_device, beam, search, ni, nn):
    """Queues of up to eight and sets of unequal size, on the crop of the furniture room (tests/beam_rooms.py: small enough for 32
    children a level, and the twin's bound stays near 1e-5 there)"""
    import beam_rooms
    from learn_region_grow_amd.lrgnet import LrgNetHIP
    small = LrgNetHIP(1, 1, ni, nn, 13, 0, device=cuda_device).load_weights(synthetic.make_synthetic_weights(**WEIGHT_KW))
    got = _followed_search(small, [beam_rooms.ml_crop_room()], beam, search, 1, np_differs=False)
    assert max(len(e) for _, _, e in got[0].beam_trace) == beam          # the queue fills


def _followed_search(net, rooms, beam, search, in_flight, np_differs=True):
    from learn_region_grow_amd.beam import BeamSearchGrower
    device = {}

    def followed(sd):
        device[sd] = BeamSearchGrower(net, rooms_in_flight=in_flight, beam_width=beam, search_width=search, seed=sd, policy='net', scoring='ml',
                                      trace=True).run(rooms)
        out = []
        for room, g in zip(rooms, device[sd]):
            try:
                out.append(_twin(net, room, sd, beam, search, 'ml', follow=g.beam_trace))
            except beam_ml_ref.FollowError as e:      # a record the twin can refute -- unless a draw within float32 noise of its confidence
                if e.result.min_rel_margin >= SAME_LOGITS_MARGIN:      # came first: then this seed is passed over, like any such seed
                    raise
                out.append(e.result)
        return out
    # the draws (not the scores) must keep their distance from the confidences, along the path that was followed: the existing rule
    seed, wants = seed_without_near_tie(followed, range(21, 29), SAME_LOGITS_MARGIN)
    got = device[seed]
    compared = undecided = 0
    for room, g, want in zip(rooms, got, wants):
        assert _regions(g) == _regions(want)
        np.testing.assert_array_equal(g.cluster_label, want.cluster_label)
        np.testing.assert_array_equal(g.filled_label, want.filled_label)
        assert [(s, l) for s, l, _ in g.beam_trace] == [(s, l) for s, l, _ in want.beam_trace]
        compared += want.pairs_compared
        undecided += want.pairs_undecided
        print('beam %d x %d room %d: %d records, %d pairs compared, %d undecided, worst relative bound %.2g' % (
            beam, search, room['room_id'], len(g.beam_trace), want.pairs_compared, want.pairs_undecided, want.worst_rel_bound))
    assert compared > 50 and undecided <= UNDECIDED_CAP * compared, '%d of %d pairs undecided' % (undecided, compared)
    # the score is exercised: 'np' ends elsewhere in at least one room
    if np_differs:
        base = BeamSearchGrower(net, rooms_in_flight=in_flight, beam_width=beam, search_width=search, seed=seed, policy='net').run(rooms)
        assert any(not np.array_equal(b.cluster_label, g.cluster_label) for b, g in zip(base, got)), "'ml' and 'np' end in the same labels"
    # and the same run again: the same labels and traces, bit for bit
    again = BeamSearchGrower(net, rooms_in_flight=in_flight, beam_width=beam, search_width=search, seed=seed, policy='net', scoring='ml',
                             trace=True).run(rooms)
    for a, g in zip(again, got):
        np.testing.assert_array_equal(a.filled_label, g.filled_label)
        assert [(s, l, [(o, n, np.float64(x).tobytes()) for o, n, x in e]) for s, l, e in a.beam_trace] == \
               [(s, l, [(o, n, np.float64(x).tobytes()) for o, n, x in e]) for s, l, e in g.beam_trace]
    return got


def test_np_with_the_trace_on(net, rooms):
    from learn_region_grow_amd.beam import BeamSearchGrower
    kw = dict(rooms_in_flight=2, beam_width=2, search_width=2, seed=21, policy='net')
    plain = BeamSearchGrower(net, **kw).run(rooms)
    traced = BeamSearchGrower(net, scoring='np', trace=True, trace_capacity=8, **kw).run(rooms)      # (a buffer this small is read out on the way)
    for p, t in zip(plain, traced):
        assert not hasattr(p, 'beam_trace') and len(t.beam_trace) > 10
        np.testing.assert_array_equal(p.cluster_label, t.cluster_label)
        np.testing.assert_array_equal(p.filled_label, t.filled_label)
        assert _regions(p) == _regions(t)
        for _, _, entries in t.beam_trace:
            assert len(entries) <= 2 and all(score == float(size) for _, size, score in entries)
            assert [size for _, size, _ in entries] == sorted((size for _, size, _ in entries), reverse=True)


def test_cli_beam_search_scoring_ml(cuda_device, tmp_path):
    """--beam 2 --search-width 2 --scoring ml end to end; the per-room lines equal the twin's, which follows the same search on the
    same files (BeamSearchGrower with the command line's arguments and the trace on)."""
    from learn_region_grow_amd.beam import BeamSearchGrower
    from learn_region_grow_amd.lrgnet import LrgNetHIP
    raw = [synthetic.area5_shaped_room(1200 + 300 * i, 60 + i, n_furniture=3).astype(np.float32) for i in range(2)]
    h5 = str(tmp_path / 'rooms.h5')
    lio.saveToH5(h5, raw)
    weights = synthetic.make_synthetic_weights(**WEIGHT_KW)
    prefix = str(tmp_path / 'lrgnet.ckpt')
    checkpoint.write_bundle(prefix, weights)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'region_grow.py'), '--h5', h5, '--ckpt', prefix, '--policy', 'gt', '--seed', '4',
                        '--beam', '2', '--search-width', '2', '--scoring', 'ml'], capture_output=True, text=True, cwd=str(tmp_path), timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    net = LrgNetHIP(1, 1, 512, 512, 13, 0, device=cuda_device).load_weights(weights)
    loaded, obj, cls = lio.loadFromH5(h5)
    pre = [preprocess_ref.preprocess_room(loaded[i], obj[i], cls[i]) for i in range(2)]
    rooms = [dict(points=p['points'], obj_id=p['obj_id'], order=np.argsort(p['curvatures']).astype(np.int32), room_id=i) for i, p in enumerate(pre)]
    traced = BeamSearchGrower(net, rooms_in_flight=2, beam_width=2, search_width=2, seed=4, policy='gt', scoring='ml', trace=True).run(rooms)
    want = []
    for i, (room, t) in enumerate(zip(rooms, traced)):
        res = beam_ml_ref.beam_room(room['points'], room['obj_id'], room['order'], None, rng_ref.CounterStream(4, i), net_fn=gpu_net_fn(net),
                                    policy='gt', beam_width=2, search_width=2, scoring='ml', follow=t.beam_trace)
        want.append(metrics.room_line('custom', i, metrics_ref.room_metrics(pre[i]['obj_id'], res.filled_label)))
    assert [ln for ln in r.stdout.splitlines() if ln.startswith('Area custom room')] == want
