"""GPU: the benchmarks.py baselines on the device (lrg_baseline_segment) against the reference script's own labels
(tests/golden/baselines_ref_cpu.npz) and the NumPy restatement (tests/baselines_ref.py): batching, predicate boundaries,
ties, a 200 k-point scene, repeatability, errors and the command line."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO
import baselines_ref as R

pytestmark = pytest.mark.gpu

MODES = ('normal', 'curvature', 'color', 'feature', 'smoothness')
ROOMS = (0, 1, 2)


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'baselines_ref_cpu.npz'))


@pytest.fixture(scope='module')
def B(hip_lib, cuda_device):
    from learn_region_grow_amd import baselines
    return baselines


@pytest.fixture(scope='module')
def rooms(golden):
    rooms = R.golden_rooms()                       # regenerated from their seeds, pinned by the golden's digest
    assert R.rooms_digest(rooms) == str(golden['rooms_digest'])
    return rooms


@pytest.fixture(scope='module')
def dev_feats(B, rooms, cuda_device):
    return [B.room_features(rooms[r], device=cuda_device) for r in ROOMS]


def _room(xyz, rgb=None, normals=None, curv=None):
    """A hand-built equalised room (features given, not computed)."""
    xyz = np.asarray(xyz, np.float32)
    n = len(xyz)
    rgb = np.zeros((n, 3), np.float32) if rgb is None else np.asarray(rgb, np.float32)
    normals = np.tile([0.0, 0.0, 1.0], (n, 1)) if normals is None else np.asarray(normals, np.float64)
    curv = np.zeros(n) if curv is None else np.asarray(curv, np.float64)
    rank = np.empty(n, np.int32)
    rank[np.argsort(curv)] = np.arange(n)
    return dict(points=np.hstack([xyz, rgb]).astype(np.float32), normals=normals, curvatures=curv, rank=rank)


def test_features_equal_restatement(dev_feats, rooms):
    for r in ROOMS:
        h = R.features(rooms[r])
        d = dev_feats[r]
        assert np.array_equal(d['equalized_idx'], h['equalized_idx']) and np.array_equal(d['unequalized_idx'], h['unequalized_idx'])
        assert np.array_equal(d['points'], h['points'])
        assert np.array_equal(d['normals'].view(np.uint64), h['normals'].view(np.uint64))
        assert np.array_equal(d['curvatures'].view(np.uint64), h['curvatures'].view(np.uint64))
        assert np.array_equal(d['rank'], h['rank'])


@pytest.mark.parametrize('mode', MODES)
def test_labels_equal_reference(B, dev_feats, golden, cuda_device, mode):
    labels, counts = B.segment(dev_feats, mode, device=cuda_device, return_counts=True)
    for r in ROOMS:
        g = golden['%s__label%d' % (mode, r)]
        assert np.array_equal(labels[r], g), (mode, r)
        assert counts[r] == g.max()


def test_batch_equals_one_at_a_time(B, dev_feats, cuda_device):
    rs = np.random.RandomState(3)
    rooms = [dev_feats[2], _room([[0.0, 0.0, 0.0]]),                                         # one point
             _room(np.arange(12)[:, None] * np.array([[0.3, 0.0, 0.0]])),                     # no edges: 3 voxels apart
             dev_feats[0], _room(np.arange(14)[:, None] * np.array([[0.1, 0.0, 0.0]]))]     # one line of 14
    for k in range(5):                                                                       # small random rooms
        xyz = np.unique(rs.randint(0, 6, size=(60, 3)), axis=0) * 0.1
        nrm = rs.normal(size=(len(xyz), 3))
        nrm = np.abs(nrm / np.linalg.norm(nrm, axis=1, keepdims=True))
        rooms.append(_room(xyz, rs.uniform(0, 1, (len(xyz), 3)), nrm, rs.uniform(0, 0.05, len(xyz))))
    for mode in MODES:
        t = B.default_thresholds(mode)
        if mode in ('normal', 'smoothness', 'feature'):
            t = (0.9,) + t[1:]
        batch = B.segment(rooms, mode, thresholds=t, device=cuda_device)
        for r, room in enumerate(rooms):
            one = B.segment([room], mode, thresholds=t, device=cuda_device)[0]
            assert np.array_equal(batch[r], one), (mode, r)
            assert np.array_equal(one, R.segment(room, mode, t)), (mode, r)
        assert (batch[1] == 0).all() and (batch[2] == 0).all() and (batch[4] == 1).all()


def test_normal_edge_follows_fma_chain(B, cuda_device):
    rs = np.random.RandomState(5)
    for _ in range(100000):
        a, b = rs.normal(size=3), rs.normal(size=3)
        a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
        plain = (b[0] * a[0] + b[1] * a[1]) + b[2] * a[2]
        fused = R.ddot3(b, a)
        if plain > fused:
            break
    else:
        pytest.fail('no pair found where the plain sum exceeds the FMA chain')
    room = _room([[0, 0, 0], [0.1, 0, 0]], normals=[a, b])
    # threshold = the FMA value: no edge (the plain sum would make one); one ulp below it: an edge
    assert B.segment([room], 'normal', thresholds=(fused, 0, 0), min_cluster_size=1, device=cuda_device)[0].tolist() == [0, 0]
    below = np.nextafter(fused, -np.inf)
    assert B.segment([room], 'normal', thresholds=(below, 0, 0), min_cluster_size=1, device=cuda_device)[0].tolist() == [1, 1]


def test_color_threshold_compared_in_float32(B, cuda_device):
    d = np.float32(0.0625)                                 # rgb 0.5 and 0.5625: the difference and its square are exact
    s = np.float32(d * d)
    t = float(s) + float(np.spacing(s)) * 0.25            # t > s in float64, float32(t) == s
    assert np.float32(t) == s and t > float(s)
    room = _room([[0, 0, 0], [0.1, 0, 0]], rgb=[[0.5, 0.5, 0.5], [0.5 + d, 0.5, 0.5]])
    assert B.segment([room], 'color', thresholds=(t, 0, 0), min_cluster_size=1, device=cuda_device)[0].tolist() == [0, 0]
    assert B.segment([room], 'color', thresholds=(float(np.nextafter(s, np.float32(1))), 0, 0), min_cluster_size=1,
                     device=cuda_device)[0].tolist() == [1, 1]


def test_curvature_difference_equal_to_threshold(B, cuda_device):
    room = _room([[0, 0, 0], [0.1, 0, 0]], curv=[0.25, 0.5])
    assert B.segment([room], 'curvature', thresholds=(0.25, 0, 0), min_cluster_size=1, device=cuda_device)[0].tolist() == [0, 0]
    assert B.segment([room], 'curvature', thresholds=(np.nextafter(0.25, 1), 0, 0), min_cluster_size=1,
                     device=cuda_device)[0].tolist() == [1, 1]


def test_smoothness_tied_curvatures(B, cuda_device):
    # planar patches of 2 .. 12 points with ONE curvature value: the ranks (host numpy.argsort, unstable) decide the seeds
    xyz = []
    for j, (a, b) in enumerate([(1, 2), (2, 2), (3, 3), (2, 5), (3, 4), (1, 11), (2, 3)]):
        for u in range(a):
            for v in range(b):
                xyz.append([0.5 * j, 0.1 * u + 3 * j, 0.1 * v])
    room = _room(xyz, curv=np.full(len(xyz), 0.125))
    for mcs in (1, 5, 10):
        lab = B.segment([room], 'smoothness', min_cluster_size=mcs, device=cuda_device)[0]
        assert np.array_equal(lab, R.segment_literal_smoothness(room, 0.98, min_cluster_size=mcs)), mcs


@pytest.fixture(scope='module')
def big_scene(B, cuda_device):
    from learn_region_grow_amd import synthetic
    raw = synthetic.area5_shaped_room(210000, 11).astype(np.float32)
    f = B.room_features(raw, device=cuda_device)
    assert len(f['points']) >= 200000
    return f


@pytest.mark.parametrize('mode', ('normal', 'smoothness'))
def test_large_scene_equals_restatement(B, big_scene, cuda_device, mode):
    lab = B.segment([big_scene], mode, device=cuda_device)[0]
    assert np.array_equal(lab, R.segment(big_scene, mode, B.default_thresholds(mode)))


def test_two_calls_identical(B, big_scene, dev_feats, cuda_device):
    rooms = [big_scene] + list(dev_feats)
    a = B.segment(rooms, 'feature', device=cuda_device)
    b = B.segment(rooms, 'feature', device=cuda_device)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_errors(B, hip_lib, cuda_device):
    import torch
    from learn_region_grow_amd import _lib
    room = _room([[0, 0, 0], [0.1, 0, 0]])
    with pytest.raises(ValueError):
        B.segment([room], 'edge', device=cuda_device)
    with pytest.raises(ValueError):
        B.segment([room], 'normal', min_cluster_size=65, device=cuda_device)
    assert hip_lib.lrg_baseline_workspace_bytes(2, 1, 65) == 0 and hip_lib.lrg_baseline_workspace_bytes(2, 1, 64) > 0
    with pytest.raises(_lib.LrgHipError, match='not equalised'):
        B.segment([_room([[0, 0, 0], [0.1, 0, 0], [0.01, 0, 0]])], 'color', device=cuda_device)
    # the C-ABI itself: unknown mode, NULL normals where the mode reads them, min_cluster_size above the cap
    pts = torch.from_numpy(room['points']).to(cuda_device)
    nrm = torch.from_numpy(room['normals']).to(cuda_device)
    starts = np.array([0, 2], np.int32)
    ws = torch.empty(hip_lib.lrg_baseline_workspace_bytes(2, 1, 10), dtype=torch.uint8, device=cuda_device)
    labels = torch.empty(2, dtype=torch.int32, device=cuda_device)
    counts = torch.empty(1, dtype=torch.int32, device=cuda_device)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def call(mode, normals, mcs=10):
        return hip_lib.lrg_baseline_segment(p(pts), 6, starts.ctypes.data_as(ctypes.c_void_p), 1, ctypes.c_float(0.1), mode, p(normals),
                                            None, None, 0.9, 0.0, 0.0, mcs, p(ws), ws.numel(), p(labels), p(counts), None)
    assert call(7, nrm) == _lib.LRG_EINVAL - 72
    assert call(0, None) == _lib.LRG_EINVAL - 74
    assert call(0, nrm, mcs=65) == _lib.LRG_EINVAL - 71
    assert call(0, nrm) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize('mode', ('smoothness', 'color'))
def test_cli_prints_reference_lines(golden, rooms, tmp_path, cuda_device, mode):
    from learn_region_grow_amd import io
    h5 = str(tmp_path / 'rooms.h5')
    io.saveToH5(h5, rooms)
    out = subprocess.run([sys.executable, os.path.join(REPO, 'baselines.py'), '--h5', h5, '--area', '5', '--mode', mode,
                          '--batch-rooms', '2', '--save', str(tmp_path / 'ply')],
                         capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.rstrip('\n').split('\n')
    assert [l for l in lines if l.startswith('Area ')] == [str(x) for x in golden[mode + '__room_lines']]
    assert lines[-1] == str(golden[mode + '__aggregate_line'])
    assert lines[0] == 'Using threshold %s resolution 0.1' % golden[mode + '__thresholds'][0]
    assert sorted(os.listdir(tmp_path / 'ply')) == ['0.ply', '1.ply', '2.ply']
