"""GPU: the FPFH mode (lrg_fpfh, lrg_baseline_segment_fpfh, baselines.fpfh / segment(..., 'fpfh')) against the NumPy twin
tests/fpfh_ref.py, stage by stage: pair-feature counts, the descriptor from the device's own counts, the labels from the device's
own histograms; hand-built rooms, repeatability, errors and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
import baselines_ref as R
import fpfh_ref as F

pytestmark = pytest.mark.gpu

FPFH_BOUND = 100 * 256 * 2.0 ** -24            # at most 256 float32 roundings on values of at most 100 (k <= 23 here)


@pytest.fixture(scope='module')
def B(hip_lib, cuda_device):
    from learn_region_grow_amd import baselines
    return baselines


@pytest.fixture(scope='module')
def feats(B, cuda_device):
    return [B.room_features(raw, device=cuda_device) for raw in R.golden_rooms()]


@pytest.fixture(scope='module')
def twins(feats):
    return [F.twin(f) for f in feats]


@pytest.fixture(scope='module')
def dev(B, feats, cuda_device):
    """(histograms, [(counts, k)]) of the three golden rooms from one call."""
    return B.fpfh(feats, device=cuda_device, return_counts=True)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_counts_equal_twin(dev, twins):
    for r, (t, (counts, k)) in enumerate(zip(twins, dev[1])):
        assert counts.dtype == np.int32 and counts.shape == (t['N'], 33) and k.dtype == np.int32
        assert np.array_equal(k, t['k']), r
        ex = t['excused']
        l1 = np.abs(counts.astype(np.int64) - t['counts32']).sum(axis=1)
        print('room %d: %d points, %d excused, %d of them differ from the twin, largest L1 %d' % (r, t['N'], ex.sum(), (l1[ex] > 0).sum(), l1.max()))
        assert np.array_equal(counts[~ex], t['counts32'][~ex]), r
        for g in range(3):
            assert np.array_equal(counts[:, 11 * g:11 * g + 11].sum(axis=1), t['pairs']), (r, g)
        assert (l1[ex] <= 2 * t['near_pairs'][ex]).all(), r


def test_descriptor_equals_float64_twin_of_device_counts(dev, twins):
    for r, (t, h, (counts, k)) in enumerate(zip(twins, dev[0], dev[1])):
        assert h.dtype == np.float32 and h.shape == (t['N'], 33)
        assert k.max() <= 23
        want = F.fpfh_from_counts(counts, k, t['I'], t['J'], t['d2'], np.float64)
        err = np.abs(h.astype(np.float64) - want).max()
        print('room %d: largest |device - float64 twin| %.3g (bound %.3g)' % (r, err, FPFH_BOUND))
        assert err <= FPFH_BOUND, (r, err)
        sums = h.reshape(-1, 3, 11).sum(axis=2)
        assert (np.abs(sums[k > 1] - 100) < 1e-3).all() and not h[k == 1].any()


@pytest.mark.parametrize('threshold', (0.985, 0.9, 0.999))
def test_labels_equal_twin_clustering_of_device_histograms(B, feats, dev, cuda_device, threshold):
    rooms = [dict(f, fpfh=h) for f, h in zip(feats, dev[0])]
    labels, counts = B.segment(rooms, 'fpfh', threshold=threshold, device=cuda_device, return_counts=True)
    for r, room in enumerate(rooms):
        want = F.segment(room['points'], room['fpfh'], threshold)
        assert np.array_equal(labels[r], want), (threshold, r)
        assert counts[r] == want.max()
        if threshold == 0.985 and r < 2:
            assert want.max() > 1
    if threshold == 0.985:                       # the default threshold, the descriptor computed by segment itself
        own = B.segment(feats, 'fpfh', device=cuda_device)
        assert all(np.array_equal(a, b) for a, b in zip(own, labels))


def test_flat_patch_is_exact(B, cuda_device):
    room = F.flat_patch()
    h, ck = B.fpfh([room], device=cuda_device, return_counts=True)
    want = np.zeros(33, np.float32)
    want[[5, 16, 27]] = 100.0
    assert (h[0] == want[None, :]).all()
    t = F.twin(room)
    assert np.array_equal(ck[0][0], t['counts32']) and np.array_equal(ck[0][1], t['k'])
    assert (B.segment([room], 'fpfh', device=cuda_device)[0] == 1).all()           # identical histograms: one cluster of 144


def _random_room(rs, n_cells, spread):
    xyz = np.unique(rs.randint(0, spread, size=(n_cells, 3)), axis=0) * 0.1 + rs.uniform(-0.02, 0.02, (1, 3))
    xyz = xyz + rs.uniform(-0.02, 0.02, xyz.shape)                       # within 0.04 of its cell's centre: one point a voxel
    nrm = rs.normal(size=xyz.shape)
    return F.make_room(xyz, np.abs(nrm / np.linalg.norm(nrm, axis=1, keepdims=True)))


def _crowded_room(rs):
    """The 125 voxels around the origin, each point pulled towards it as far as its voxel allows (0.151 for cell 2, 0.051 for cell 1):
    the centre point has 80 neighbours and the inner points more: above what a stored neighbour list holds (48), so their gather
    probes the window again, while the outer points' lists fit."""
    cells = np.array(F.WINDOW)
    xyz = np.sign(cells) * np.maximum(np.abs(cells) * 0.1 - 0.049, 0.0)
    nrm = rs.normal(size=xyz.shape)
    return F.make_room(xyz, np.abs(nrm / np.linalg.norm(nrm, axis=1, keepdims=True)))


def _check_room(h, counts, k, room):
    t = F.twin(room)
    assert np.array_equal(k, t['k'])
    ex = t['excused']
    assert np.array_equal(counts[~ex], t['counts32'][~ex])
    want = F.fpfh_from_counts(counts, k, t['I'], t['J'], t['d2'], np.float64)
    assert np.abs(h.astype(np.float64) - want).max() <= FPFH_BOUND


def test_hand_built_rooms(B, cuda_device):
    rs = np.random.RandomState(4)
    one = F.make_room([[0.3, 0.2, 0.1]])
    two = F.make_room([[0, 0, 0], [0.1, 0.02, 0.01]], normals=[[0, 0, 1], [0, 0.6, 0.8]])
    big = _random_room(rs, 400, 8)                        # 257 .. 400 points: two workgroups
    big = dict(points=big['points'][:257], normals=big['normals'][:257])
    empty = dict(points=np.zeros((0, 6), np.float32), normals=np.zeros((0, 3)))
    a = _random_room(rs, 90, 5)
    b = dict(points=a['points'].copy(), normals=a['normals'][::-1].copy())        # the same coordinates, other normals
    crowded = _crowded_room(rs)
    rooms = [one, two, empty, big, a, b, crowded]
    assert len(big['points']) == 257
    h, ck = B.fpfh(rooms, device=cuda_device, return_counts=True)
    assert not h[0].any() and ck[0][1].tolist() == [1] and not ck[0][0].any()
    assert ck[1][1].tolist() == [2, 2] and ck[1][0].sum(axis=1).tolist() == [3, 3]
    assert h[2].shape == (0, 33) and ck[2][0].shape == (0, 33) and ck[2][1].shape == (0,)
    for r in (1, 3, 4, 5, 6):
        _check_room(h[r], ck[r][0], ck[r][1], rooms[r])
    assert ck[6][1][62] == 81 and (ck[6][1] - 1 > 48).any() and (ck[6][1] - 1 <= 48).any()      # lists that overflow and lists that do not
    assert _same(B.fpfh([crowded], device=cuda_device, lists=False)[0], h[6])
    assert not _same(h[4], h[5])                          # neighbours did not cross into the room with the same coordinates
    for r in (0, 1, 3, 4, 5, 6):                          # each equals its own solo run, byte for byte
        hs, cks = B.fpfh([rooms[r]], device=cuda_device, return_counts=True)
        assert _same(hs[0], h[r]) and _same(cks[0][0], ck[r][0]) and _same(cks[0][1], ck[r][1]), r
    labels = B.segment(rooms, 'fpfh', threshold=0.9, min_cluster_size=1, device=cuda_device)
    for r, room in enumerate(rooms):
        assert np.array_equal(labels[r], F.segment(room['points'], h[r], 0.9, min_cluster_size=1)), r
        assert np.array_equal(labels[r], B.segment([room], 'fpfh', threshold=0.9, min_cluster_size=1, device=cuda_device)[0]), r
    assert labels[0].tolist() == [0] and labels[2].shape == (0,)


def test_repeatable_and_independent_of_batch_and_lists(B, feats, dev, cuda_device):
    again = B.fpfh(feats, device=cuda_device, return_counts=True)
    probes = B.fpfh(feats, device=cuda_device, return_counts=True, lists=False)      # the gather pass probing the window again
    for r in range(len(feats)):
        for other in (again, probes):
            assert _same(other[0][r], dev[0][r]) and _same(other[1][r][0], dev[1][r][0]) and _same(other[1][r][1], dev[1][r][1]), r
    alone = B.fpfh([feats[2]], device=cuda_device)
    assert _same(alone[0], dev[0][2])
    swapped = B.fpfh([feats[2], feats[0]], device=cuda_device)
    assert _same(swapped[0], dev[0][2]) and _same(swapped[1], dev[0][0])


def test_errors(B, hip_lib, feats, cuda_device):
    import ctypes
    import torch
    from learn_region_grow_amd import _lib
    room = F.flat_patch()
    with pytest.raises(ValueError, match='radius'):
        B.fpfh([room], resolution=0.1, radius=0.2001, device=cuda_device)
    with pytest.raises(ValueError, match='normals'):
        B.fpfh([dict(points=room['points'], normals=None)], device=cuda_device)
    with pytest.raises(ValueError, match='normals'):
        B.segment([dict(points=room['points'], normals=None)], 'fpfh', device=cuda_device)
    with pytest.raises(ValueError):
        B.segment([room], 'edge', device=cuda_device)
    with pytest.raises(ValueError, match='verified'):
        B.segment([dict(room, normal_slack=np.zeros(144), curv_slack=np.zeros(144))], 'fpfh', device=cuda_device)
    dup = F.make_room([[0, 0, 0], [0.1, 0, 0], [0.01, 0, 0]])
    with pytest.raises(_lib.LrgHipError, match='not equalised'):
        B.fpfh([dup], device=cuda_device)
    with pytest.raises(_lib.LrgHipError, match='not equalised'):
        B.segment([dict(dup, fpfh=np.ones((3, 33), np.float32))], 'fpfh', device=cuda_device)
    # the C ABI itself
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    pts = torch.from_numpy(room['points']).to(cuda_device)
    xyz = torch.from_numpy(np.ascontiguousarray(room['points'][:, :3])).to(cuda_device)
    nrm = torch.from_numpy(room['normals'].astype(np.float32)).to(cuda_device)
    n = len(room['points'])
    starts = np.array([0, n], np.int32)
    ws = torch.empty(hip_lib.lrg_fpfh_workspace_bytes(n, 1, 0), dtype=torch.uint8, device=cuda_device)
    counts = torch.empty((n, 33), dtype=torch.int32, device=cuda_device)
    k = torch.empty(n, dtype=torch.int32, device=cuda_device)
    out = torch.empty((n, 33), dtype=torch.float32, device=cuda_device)

    def call(radius, ws_bytes=ws.numel(), flags=0):
        return hip_lib.lrg_fpfh(p(pts), 6, p(xyz), p(nrm), starts.ctypes.data_as(ctypes.c_void_p), 1, ctypes.c_float(0.1), ctypes.c_float(radius),
                                flags, p(ws), ws_bytes, p(counts), p(k), p(out), None)
    assert call(0.25) == _lib.LRG_EINVAL
    assert call(0.2, ws_bytes=ws.numel() - 1) == _lib.LRG_EINVAL - 93
    assert call(0.2, flags=2) == _lib.LRG_EINVAL - 90
    assert hip_lib.lrg_fpfh_workspace_bytes(n, 1, 2) == 0 and hip_lib.lrg_fpfh_workspace_bytes(n, 1, 1) > ws.numel()
    assert hip_lib.lrg_baseline_fpfh_workspace_bytes(n, 1, 10) >= hip_lib.lrg_baseline_workspace_bytes(n, 1, 10) + n * 33 * 8
    assert call(0.2) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy()[:, [5, 16, 27]] == 100).all()


def test_cli_prints_reference_lines(B, feats, tmp_path, cuda_device):
    from learn_region_grow_amd import io, metrics
    rooms = R.golden_rooms()
    h5 = str(tmp_path / 'rooms.h5')
    io.saveToH5(h5, rooms)
    out = subprocess.run([sys.executable, os.path.join(REPO, 'baselines.py'), '--h5', h5, '--area', '5', '--mode', 'fpfh',
                          '--batch-rooms', '2', '--save', str(tmp_path / 'ply')],
                         capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.rstrip('\n').split('\n')
    assert lines[0] == 'Using threshold 0.985 resolution 0.1'
    labels = B.segment(feats, 'fpfh', device=cuda_device)
    ms = [metrics.room_metrics(raw[:, 6].astype(np.int64)[f['equalized_idx']], lab.astype(np.int64)) for raw, f, lab in zip(rooms, feats, labels)]
    assert [l for l in lines if l.startswith('Area ')] == [metrics.room_line('5', r, m) for r, m in enumerate(ms)]
    assert lines[-1] == metrics.aggregate_line(ms)
    assert len([l for l in lines if l.endswith('s') and ' points: ' in l]) == 3
    assert sorted(os.listdir(tmp_path / 'ply')) == ['0.ply', '1.ply', '2.ply']
    dev_lines = subprocess.run([sys.executable, os.path.join(REPO, 'baselines.py'), '--h5', h5, '--area', '5', '--mode', 'fpfh', '--metrics', 'device'],
                               capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert dev_lines.returncode == 0, dev_lines.stderr[-2000:]
    keep = lambda text: [l for l in text.rstrip('\n').split('\n') if ' points: ' not in l and not l.startswith('Saved to ')]
    assert keep(dev_lines.stdout) == keep(out.stdout)
