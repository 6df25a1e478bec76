"""GPU: benchmarks.py --mode edge (lrg_edge_logits, lrg_edge_sigmoid, lrg_edge_segment, lrg_baseline_segment_mask, edge.segment)
against the NumPy twin tests/edge_ref.py, stage by stage and bit for bit; the device logistic function within its bound; hand-made
rooms, batching, the search cap, repeatability and errors."""
import ctypes

import numpy as np
import pytest
from scipy.special import expit

from conftest import GOLDEN
import baselines_ref
import edge_ref as T

pytestmark = pytest.mark.gpu

# The device p = 1 / (1 + exp(-z)) against scipy.special.expit(z), in units in the last place of the float64 result.  No document of
# the device library's exp error is installed with ROCm here, so the bound is twice the largest distance measured over every edge of
# rooms A and B on an MI355X (2 ulp: DESIGN.md §3.16).
DEVICE_P_ULPS = 4


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _ulps(a, b):
    """Distance in representable float64 values between non-negative a and b (NaN positions must agree)."""
    nan = np.isnan(a)
    assert np.array_equal(nan, np.isnan(b))
    d = np.abs(a[~nan].view(np.int64) - b[~nan].view(np.int64))
    return int(d.max()) if d.size else 0


@pytest.fixture(scope='module')
def E(hip_lib, cuda_device):
    from learn_region_grow_amd import edge
    return edge


@pytest.fixture(scope='module')
def weights():
    return T.golden_weights()


@pytest.fixture(scope='module')
def model(E, weights, cuda_device):
    return E.EdgeModelHIP(weights, device=cuda_device)


@pytest.fixture(scope='module')
def rooms():
    return [T.equalise(r) for r in T.raw_rooms()]


@pytest.fixture(scope='module')
def twins(rooms, weights):
    return [T.staged(r['points'], weights) for r in rooms]


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLDEN + '/edge_ref_cpu.npz') as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def dev_logits(E, model, rooms):
    return E.logits(rooms, model, return_bounds=True)


@pytest.fixture(scope='module')
def dev_stages(E, model, rooms, twins):
    """The stages after the logistic function on the twin's own p."""
    return E.segment_probabilities(rooms, [t['p'] for t in twins], model)


def test_rooms_are_the_preprocessed_ones(rooms, cuda_device):
    from learn_region_grow_amd import baselines
    for raw, r in zip(T.raw_rooms(), rooms):
        assert _same(baselines.room_features(raw, need_normals=False, device=cuda_device)['points'], r['points'])


def test_bounds_equal_twin(dev_logits, twins):
    _, nmin, nmax = dev_logits
    for r, t in enumerate(twins):
        assert _same(nmin[r], t['nmin']) and _same(nmax[r], t['nmax']), r


def test_logits_equal_twin_bit_for_bit(dev_logits, twins, golden):
    for r, (t, name) in enumerate(zip(twins, 'AB')):
        z = dev_logits[0][r]
        assert np.array_equal(np.isnan(z), t['nb'][:, 13:] < 0), r
        assert _same(z, t['z']), (r, np.nanmax(np.abs(z - t['z'])))
        assert T.digest(z) == str(golden['z_digest_' + name])


def test_keep_words_clusters_and_stop_equal_twin(dev_stages, twins):
    labels, counts, stats = dev_stages
    for r, t in enumerate(twins):
        assert _same(stats['keep'][r], t['keep']), r
        assert np.array_equal(stats['cluster_labels'][r], t['cluster_labels']) and counts[r] == t['n_clusters'], r
        assert _same(stats['stop'][r], t['stop']), r
        assert np.array_equal(labels[r], t['labels']), r
    assert stats['overflowed'] == 0
    assert stats['searches'] == sum(int((t['stop'] >= 0).sum()) for t in twins)
    assert stats['dead'] == sum(int(((t['cluster_labels'] == 0) & ~t['live']).sum()) for t in twins)
    assert stats['largest_visited'] == max(t['largest_visited'] for t in twins)


def test_components_of_given_keep_words(E, model, rooms, twins):
    labels, counts = E.components(rooms, [t['keep'] for t in twins], model)
    for r, t in enumerate(twins):
        assert np.array_equal(labels[r], t['cluster_labels']) and counts[r] == t['n_clusters'], r


def test_host_sigmoid_labels_equal_golden(E, model, rooms, golden):
    labels, counts, stats = E.segment(rooms, model, return_counts=True, return_stats=True)
    for r, name in enumerate('AB'):
        assert labels[r].dtype == np.int32
        assert np.array_equal(labels[r], golden['labels_' + name]), name
        assert counts[r] == golden['n_clusters_' + name]
    assert stats['overflowed'] == 0
    # segment() runs lrg_edge_segment on the workspace lrg_edge_logits prepared; segment_probabilities() prepares its own
    own = E.segment_probabilities(rooms, E.probabilities(rooms, model), model)
    assert all(_same(x, y) for x, y in zip(labels, own[0])) and all(_same(x, y) for x, y in zip(stats['stop'], own[2]['stop']))
    assert stats['largest_visited'] == own[2]['largest_visited'] and stats['dead'] == own[2]['dead']


def test_device_sigmoid_within_bound_and_labels_follow_its_p(E, model, rooms, twins, weights):
    p_dev = E.probabilities(rooms, model, sigmoid='device')
    worst = max(_ulps(p, expit(t['z'])) for p, t in zip(p_dev, twins))
    print('device p: largest distance from expit %d ulp (bound %d)' % (worst, DEVICE_P_ULPS))
    assert worst <= DEVICE_P_ULPS
    labels, counts = E.segment(rooms, model, sigmoid='device', return_counts=True)
    for r, room in enumerate(rooms):
        want = T.staged(room['points'], weights, p=p_dev[r])
        assert np.array_equal(labels[r], want['labels']) and counts[r] == want['n_clusters'], r


def _room(xyz, rgb=(0.5, 0.5, 0.5)):
    xyz = np.asarray(xyz, dtype=np.float32)
    return dict(points=np.ascontiguousarray(np.hstack([xyz, np.broadcast_to(np.asarray(rgb, np.float32), (len(xyz), 3))]).astype(np.float32)))


def _check_against_both_twins(E, model, weights, room, **kw):
    lit = T.literal(room['points'], weights, **kw)
    st = T.staged(room['points'], weights, **kw)
    assert np.array_equal(lit['labels'], st['labels'])
    z, = E.logits([room], model, resolution=kw.get('resolution', 0.1))
    assert _same(z, st['z'])
    labels, counts, stats = E.segment([room], model, return_counts=True, return_stats=True, **kw)
    assert np.array_equal(labels[0], lit['labels']) and counts[0] == lit['n_clusters']
    assert _same(stats['stop'][0], st['stop']) and _same(stats['keep'][0], st['keep'])
    return st


def test_two_points(E, model, weights):
    st = _check_against_both_twins(E, model, weights, _room([[0.0, 0.0, 0.0], [0.1, 0.1, 0.0]]))
    assert (st['nb'] >= 0).sum() == 2


def test_room_without_neighbour_pairs(E, model, weights):
    room = _room([[0.5 * i, 0.3 * i, 0.0] for i in range(7)])
    st = _check_against_both_twins(E, model, weights, room)
    assert not (st['nb'] >= 0).any() and not st['labels'].any()
    z, = E.logits([room], model)
    assert np.isnan(z).all()


def test_patch_of_one_colour_is_decided_by_the_tie_key(E, model, weights):
    # voxels of 0.125 m: the coordinates and their differences are exact in float32, so the edges of an interior point to opposite
    # neighbours have the same features and the same probability to the last bit
    room = _room([[0.125 * i, 0.125 * j, 1.0] for i in range(12) for j in range(12)])
    for mcs in (10, 64):                           # 64: most of the patch has to be searched
        st = _check_against_both_twins(E, model, weights, room, min_cluster_size=mcs, resolution=0.125)
    pe = np.where(st['nb'] >= 0, T.edge_probs(st['p'], st['nb']), -1.0)
    ties = sum(len(row[row >= 0]) - len(np.unique(row[row >= 0])) for row in pe)
    assert ties > 100


def test_cluster_of_exactly_min_cluster_size_is_not_kept(E, model):
    mcs = 10
    room = _room([[0.1 * i, 0.0, 0.0] for i in range(mcs)] + [[0.1 * i, 5.0, 0.0] for i in range(mcs + 1)])
    nb = baselines_ref.neighbours(room['points'], 0.1)
    p = np.where(nb[:, 13:] >= 0, 1.0, np.nan)
    labels, counts, stats = E.segment_probabilities([room], [p], model, min_cluster_size=mcs)
    assert counts[0] == 1 and not labels[0][:mcs].any() and (labels[0][mcs:] == 1).all()
    assert stats['dead'] == mcs and stats['searches'] == 0


def test_batch_equals_rooms_alone(E, model, rooms, weights, golden):
    tiny = _room([[0.1 * i, 0.1 * j, 0.0] for i in range(5) for j in range(4)], rgb=(0.2, 0.6, 0.4))
    batch = [rooms[0], rooms[1], tiny, rooms[0]]                      # the last shares every voxel coordinate with the first
    labels, counts = E.segment(batch, model, return_counts=True)
    zs = E.logits(batch, model)
    for r, room in enumerate(batch):
        alone, c = E.segment([room], model, return_counts=True)
        assert np.array_equal(labels[r], alone[0]) and counts[r] == c[0], r
        assert _same(zs[r], E.logits([room], model)[0]), r
    assert np.array_equal(labels[0], golden['labels_A']) and np.array_equal(labels[3], golden['labels_A'])
    assert np.array_equal(labels[2], T.literal(tiny['points'], weights)['labels'])


def test_small_search_cap_overflows_and_the_host_finishes(E, model, rooms, twins, golden):
    labels, counts, stats = E.segment(rooms[:1], model, search_cap=8, return_counts=True, return_stats=True)
    capped = T.staged(rooms[0]['points'], T.golden_weights(), cap=8)
    assert stats['overflowed'] == int((capped['stop'] == -2).sum()) > 0
    assert np.array_equal(labels[0], golden['labels_A'])
    assert _same(stats['stop'][0], twins[0]['stop'])
    assert stats['largest_visited'] == twins[0]['largest_visited']


def test_two_calls_give_identical_labels(E, model, rooms):
    for sig in ('host', 'device'):
        a = E.segment(rooms, model, sigmoid=sig)
        b = E.segment(rooms, model, sigmoid=sig)
        assert all(_same(x, y) for x, y in zip(a, b))


def test_unequalised_room_is_refused(E, model, rooms):
    from learn_region_grow_amd import _lib
    pts = rooms[0]['points'][:50].copy()
    bad = dict(points=np.vstack([pts, pts[7:8]]))
    with pytest.raises(_lib.LrgHipError, match='not equalised'):
        E.segment([bad], model)
    with pytest.raises(_lib.LrgHipError, match='not equalised'):
        E.logits([bad], model)


def test_bad_arguments_return_einval(E, model, hip_lib, cuda_device):
    import torch
    from learn_region_grow_amd import _lib
    n = 4
    pts = torch.zeros((n, 6), dtype=torch.float32, device=cuda_device)
    pts[:, 0] = torch.arange(n, device=cuda_device) * 0.1
    rs = np.array([0, n], dtype=np.int32)
    rsp = rs.ctypes.data_as(ctypes.c_void_p)
    nbytes = hip_lib.lrg_edge_workspace_bytes(n, 1, 10, 1024)
    assert nbytes > 0
    assert hip_lib.lrg_edge_workspace_bytes(-1, 1, 10, 1024) == 0 and hip_lib.lrg_edge_workspace_bytes(n, 1, 0, 1024) == 0
    assert hip_lib.lrg_edge_workspace_bytes(n, 1, 10, 0) == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda_device)
    z = torch.empty((n, 13), dtype=torch.float64, device=cuda_device)
    out = torch.empty(n, dtype=torch.int32, device=cuda_device)
    cnt = torch.empty(4, dtype=torch.int32, device=cuda_device)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    res = ctypes.c_float(0.1)

    def einval(rc):
        return _lib.LRG_EINVAL - 100 < rc <= _lib.LRG_EINVAL
    lg = hip_lib.lrg_edge_logits
    assert einval(lg(P(pts), 6, None, 1, res, P(model.packed), P(ws), nbytes, P(z), None, None, None))          # no room_start
    assert einval(lg(None, 6, rsp, 1, res, P(model.packed), P(ws), nbytes, P(z), None, None, None))             # no points
    assert einval(lg(P(pts), 5, rsp, 1, res, P(model.packed), P(ws), nbytes, P(z), None, None, None))           # ld < 6
    assert einval(lg(P(pts), 6, rsp, 1, res, None, P(ws), nbytes, P(z), None, None, None))                      # no weights
    assert einval(lg(P(pts), 6, rsp, 1, res, P(model.packed), None, nbytes, P(z), None, None, None))            # no workspace
    assert einval(lg(P(pts), 6, rsp, 1, res, P(model.packed), P(ws), 16, P(z), None, None, None))               # workspace too small
    assert einval(lg(P(pts), 6, rsp, 1, res, P(model.packed), P(ws), nbytes, None, None, None, None))           # no output
    assert einval(lg(P(pts), 6, rsp, 1, ctypes.c_float(0.0), P(model.packed), P(ws), nbytes, P(z), None, None, None))
    bad = np.array([0, 3, 2], dtype=np.int32)
    assert einval(lg(P(pts), 6, bad.ctypes.data_as(ctypes.c_void_p), 2, res, P(model.packed), P(ws), nbytes, P(z), None, None, None))
    assert einval(hip_lib.lrg_edge_sigmoid(None, 4, P(z), None)) and einval(hip_lib.lrg_edge_sigmoid(P(z), -1, P(z), None))
    sg = hip_lib.lrg_edge_segment
    assert einval(sg(P(pts), 6, rsp, 1, res, None, 0.99, 0.9, 10, 1024, P(ws), nbytes, P(out), P(out), P(out), P(cnt), None, None, 0, None))
    assert einval(sg(P(pts), 6, rsp, 1, res, P(z), 0.99, 0.9, 10, 1024, P(ws), nbytes, None, P(out), P(out), P(cnt), None, None, 0, None))
    assert einval(sg(P(pts), 6, rsp, 1, res, P(z), 0.99, 0.9, 10, 1024, P(ws), nbytes - 256, P(out), P(out), P(out), P(cnt), None, None, 0, None))
    assert einval(sg(P(pts), 6, rsp, 1, res, P(z), 0.99, 0.9, 0, 1024, P(ws), nbytes, P(out), P(out), P(out), P(cnt), None, None, 0, None))
    assert einval(sg(P(pts), 6, rsp, 1, res, P(z), 0.99, 0.9, 10, 0, P(ws), nbytes, P(out), P(out), P(out), P(cnt), None, None, 0, None))
    assert einval(sg(P(pts), 6, rsp, 1, res, P(z), float('nan'), 0.9, 10, 1024, P(ws), nbytes, P(out), P(out), P(out), P(cnt), None, None, 0, None))
    bws = torch.empty(hip_lib.lrg_baseline_workspace_bytes(n, 1, 10), dtype=torch.uint8, device=cuda_device)
    assert einval(hip_lib.lrg_baseline_segment_mask(P(pts), 6, rsp, 1, res, None, 10, P(bws), bws.numel(), P(out), P(out), None))
    assert einval(hip_lib.lrg_edge_status(None, None, None))
    torch.cuda.synchronize()


def test_cli_prints_reference_lines(E, model, rooms, golden, tmp_path):
    import os
    import subprocess
    import sys
    from conftest import REPO
    from learn_region_grow_amd import io, metrics
    raw = T.raw_rooms()
    h5 = str(tmp_path / 'rooms.h5')
    io.saveToH5(h5, raw)
    ckpt = os.path.join(GOLDEN, 'edge5_weights.npz')
    out = subprocess.run([sys.executable, os.path.join(REPO, 'edge.py'), '--h5', h5, '--area', '5', '--ckpt', ckpt, '--metrics', 'device',
                          '--save', str(tmp_path / 'ply')], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.rstrip('\n').split('\n')
    assert lines[0] == 'Restored from %s' % ckpt
    ms = [metrics.room_metrics(r[:, 6].astype(np.int64)[room['equalized_idx']], golden['labels_' + name].astype(np.int64))
          for r, room, name in zip(raw, rooms, 'AB')]
    assert [l for l in lines if l.startswith('Area ')] == [metrics.room_line('5', r, m) for r, m in enumerate(ms)]
    assert lines[-1] == metrics.aggregate_line(ms)
    assert len([l for l in lines if l.endswith('s') and ' points: ' in l]) == 2
    assert sorted(os.listdir(tmp_path / 'ply')) == ['0.ply', '1.ply']
