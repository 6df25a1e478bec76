"""GPU: the baselines' features solved on the device (lrg_baseline_eig) and the edge certificate (lrg_baseline_certify): labels and
rank of room_features(eig='verified') + segment equal the 'lapack' route's, the solver bound holds, thresholds placed on an edge,
the certificate kernel on hand-made rooms against its NumPy restatement, the old route untouched, and the redone share stays small."""
import copy
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLDEN
import baselines_ref as R
import baselines_verified_ref as V

pytestmark = pytest.mark.gpu

MODES = ('normal', 'curvature', 'color', 'feature', 'smoothness')
ROOMS = (0, 1, 2)


@pytest.fixture(scope='module')
def B(hip_lib, cuda_device):
    from learn_region_grow_amd import baselines
    return baselines


@pytest.fixture(scope='module')
def raw_rooms():
    return R.golden_rooms()


@pytest.fixture(scope='module')
def lap(B, raw_rooms, cuda_device):
    """The 'lapack' route's features: the reference of every comparison here.  Never modified."""
    return [B.room_features(raw_rooms[r], device=cuda_device) for r in ROOMS]


@pytest.fixture(scope='module')
def ver(B, raw_rooms, cuda_device):
    """The 'verified' route's features as room_features returns them.  segment() completes such dicts in place: tests take copies."""
    return [B.room_features(raw_rooms[r], device=cuda_device, eig='verified') for r in ROOMS]


@pytest.fixture(scope='module')
def lap_labels(B, lap, cuda_device):
    return {mode: B.segment(lap, mode, device=cuda_device) for mode in MODES}


def test_rank_and_layout(lap, ver):
    for r in ROOMS:
        v, l = ver[r], lap[r]
        n = len(l['points'])
        assert np.array_equal(v['points'], l['points']) and np.array_equal(v['equalized_idx'], l['equalized_idx'])
        assert np.array_equal(v['unequalized_idx'], l['unequalized_idx'])
        assert v['rank'].dtype == np.int32 and np.array_equal(v['rank'], l['rank']), r
        assert v['cov'].shape == (n, 9) and v['cov'].dtype == np.float64
        assert v['normals'].shape == (n, 3) and v['curvatures'].shape == (n,)
        assert v['normal_slack'].shape == (n,) and v['curv_slack'].shape == (n,)
        assert np.isfinite(v['normal_slack']).all() and np.isfinite(v['curv_slack']).all()      # the unbounded points were redone
        exact = v['curv_slack'] == 0
        assert np.array_equal(v['normals'][exact].view(np.uint64), l['normals'][exact].view(np.uint64))
        assert np.array_equal(v['curvatures'][exact].view(np.uint64), l['curvatures'][exact].view(np.uint64))
        s = v['verify_stats']
        assert s['points'] == n and s['rank_redone'] + s['degenerate'] == int(exact.sum())
        assert 'normal_slack' not in l and 'verify_stats' not in l


@pytest.mark.parametrize('mode', MODES)
def test_labels_equal_lapack_route(B, ver, lap_labels, cuda_device, mode):
    want = lap_labels[mode]
    for r in ROOMS:
        got, cnt = B.segment([copy.deepcopy(ver[r])], mode, device=cuda_device, return_counts=True)
        assert np.array_equal(got[0], want[r]), (mode, r)
        assert cnt[0] == want[r].max()
    batch = B.segment(copy.deepcopy(ver), mode, device=cuda_device)
    for r in ROOMS:
        assert np.array_equal(batch[r], want[r]), (mode, 'batch', r)


def _device_solve(hip_lib, cuda_device, cov):
    import torch
    n = len(cov)
    c = torch.from_numpy(np.ascontiguousarray(cov)).to(cuda_device)
    nrm = torch.empty((n, 3), dtype=torch.float64, device=cuda_device)
    out = torch.empty((3, n), dtype=torch.float64, device=cuda_device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert hip_lib.lrg_baseline_eig(p(c), n, p(nrm), p(out[0]), p(out[1]), p(out[2]), None) == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return nrm.cpu().numpy(), o[0], o[1], o[2]


def test_solver_bound(hip_lib, cuda_device, lap, ver):
    """Every value lrg_baseline_eig bounds lies within its slack of LAPACK's.  The ratios are measurements (printed; DESIGN.md §3.8
    records them); the assertion is the bound itself."""
    for r in ROOMS:
        nrm, c, ns, cs = _device_solve(hip_lib, cuda_device, ver[r]['cov'])
        ok = np.isfinite(ns)
        assert np.array_equal(ok, np.isfinite(cs))
        assert ok.any() and (ns[ok] > 0).all() and (cs[ok] == 256.0 * np.finfo(np.float64).eps).all()
        rn = float((np.abs(nrm[ok] - lap[r]['normals'][ok]) / ns[ok, None]).max())
        rc = float((np.abs(c[ok] - lap[r]['curvatures'][ok]) / cs[ok]).max())
        print('room %d: %d of %d points bounded; largest |normal - LAPACK| / normal_slack = %.4f, |curvature - LAPACK| / curv_slack = %.4f'
              % (r, int(ok.sum()), len(ok), rn, rc))
        assert rn <= 1.0 and rc <= 1.0, (r, rn, rc)
        # what room_features kept from the device is this solve
        kept = ver[r]['curv_slack'] > 0
        assert np.array_equal(ver[r]['normals'][kept].view(np.uint64), nrm[kept].view(np.uint64))
        assert np.array_equal(ver[r]['curvatures'][kept].view(np.uint64), c[kept].view(np.uint64))
        assert np.array_equal(ver[r]['normal_slack'][kept], ns[kept])


def _device_pair(room):
    """A 26-neighbour pair (i, k), k < i, whose two ends still hold the device's values (finite, non-zero slack)."""
    nb = R.neighbours(room['points'], 0.1)
    dev = (room['normal_slack'] > 0) & np.isfinite(room['normal_slack']) & (room['curv_slack'] > 0)
    for i in range(len(nb) // 2, len(nb)):
        for k in nb[i]:
            if 0 <= k < i and dev[i] and dev[k] and room['curvatures'][i] != room['curvatures'][k]:
                return i, int(k)
    pytest.fail('no pair of device-valued neighbours')


def test_threshold_on_an_edge(B, lap, ver, cuda_device):
    i, k = _device_pair(ver[0])
    d = R.ddot3(ver[0]['normals'][k], ver[0]['normals'][i])
    dc = abs(ver[0]['curvatures'][k] - ver[0]['curvatures'][i])
    for mode, t in (('normal', d), ('curvature', dc)):
        room = copy.deepcopy(ver[0])
        got, stats = B.segment([room], mode, threshold=t, device=cuda_device, return_stats=True)
        flags = stats['flags'][0]
        assert flags[i] and flags[k], (mode, t)
        assert stats['flagged'][0] == flags.sum() >= 2
        # the flagged points now hold LAPACK's values, the others were left alone
        assert (room['normal_slack'][flags] == 0).all() and (room['curv_slack'][flags] == 0).all()
        assert np.array_equal(room['normals'][flags].view(np.uint64), lap[0]['normals'][flags].view(np.uint64))
        assert np.array_equal(room['curvatures'][flags].view(np.uint64), lap[0]['curvatures'][flags].view(np.uint64))
        assert np.array_equal(room['normals'][~flags].view(np.uint64), ver[0]['normals'][~flags].view(np.uint64))
        assert np.array_equal(room['rank'], ver[0]['rank'])
        want = B.segment([lap[0]], mode, threshold=t, device=cuda_device)[0]
        assert np.array_equal(got[0], want), mode


def test_certificate_kernel_on_handmade_rooms(hip_lib, cuda_device):
    import torch
    rooms, expected = V.handmade()
    sizes = [len(r['points']) for r in rooms]
    starts = np.array([0, sizes[0], sizes[0] + sizes[1]], dtype=np.int32)
    n = int(starts[-1])
    assert sizes == [28, 5] and starts[1] % 64 and n < 256
    dev = lambda key: torch.from_numpy(np.ascontiguousarray(np.concatenate([r[key] for r in rooms]))).to(cuda_device)
    pts, nrm, cur, ns, cs = dev('points'), dev('normals'), dev('curvatures'), dev('normal_slack'), dev('curv_slack')
    ws = torch.empty(hip_lib.lrg_baseline_workspace_bytes(n, 2, 10), dtype=torch.uint8, device=cuda_device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for mode in MODES:
        t = V.thresholds(mode)
        flags = torch.full((n,), 7, dtype=torch.int32, device=cuda_device)
        count = torch.full((1,), 7, dtype=torch.int32, device=cuda_device)
        rc = hip_lib.lrg_baseline_certify(p(pts), 6, starts.ctypes.data_as(ctypes.c_void_p), 2, ctypes.c_float(0.1), MODES.index(mode), p(nrm),
                                          p(cur), p(ns), p(cs), t[0], t[1], t[2], 10, p(ws), ws.numel(), p(flags), p(count), None)
        assert rc == 0, (mode, rc)
        status = ctypes.c_int32(-1)
        assert hip_lib.lrg_baseline_status(p(ws), n, 2, 10, ctypes.byref(status), None) == 0 and status.value == 0
        got = flags.cpu().numpy()
        want = np.concatenate([V.certify(room, mode, t) for room in rooms])
        assert np.array_equal(want, np.concatenate(expected[mode])), mode
        assert set(got.tolist()) <= {0, 1}
        assert np.array_equal(got.astype(bool), want), (mode, np.nonzero(got.astype(bool) != want)[0])
        assert int(count.item()) == int(want.sum()), mode
    # the embedding mode has no certificate; the outputs are required
    assert hip_lib.lrg_baseline_certify(p(pts), 6, starts.ctypes.data_as(ctypes.c_void_p), 2, ctypes.c_float(0.1), 5, p(nrm), p(cur), p(ns), p(cs),
                                        0.5, 0.0, 0.0, 10, p(ws), ws.numel(), p(flags), p(count), None) != 0
    assert hip_lib.lrg_baseline_certify(p(pts), 6, starts.ctypes.data_as(ctypes.c_void_p), 2, ctypes.c_float(0.1), 0, p(nrm), p(cur), p(ns), p(cs),
                                        0.5, 0.0, 0.0, 10, p(ws), ws.numel(), None, p(count), None) != 0
    assert hip_lib.lrg_baseline_certify(p(pts), 6, starts.ctypes.data_as(ctypes.c_void_p), 2, ctypes.c_float(0.1), 0, p(nrm), p(cur), None, p(cs),
                                        0.5, 0.0, 0.0, 10, p(ws), ws.numel(), p(flags), p(count), None) != 0
    torch.cuda.synchronize()


def test_segment_flags_handmade_rooms(B, cuda_device):
    """segment() on dicts that carry slacks runs the certificate with ITS mode and thresholds and reports the flags per room."""
    for mode in MODES:
        rooms, expected = V.handmade()
        for room in rooms:                                          # LAPACK's values for a flagged point come from room['cov']
            room['cov'] = np.tile(np.diag([3.0, 2.0, 1.0]).reshape(9), (len(room['points']), 1))
        _, stats = B.segment(rooms, mode, thresholds=V.thresholds(mode), min_cluster_size=1, device=cuda_device, return_stats=True)
        for r in range(2):
            assert np.array_equal(stats['flags'][r], expected[mode][r]), (mode, r)
            assert stats['flagged'][r] == expected[mode][r].sum()
            f = expected[mode][r]
            assert (rooms[r]['normals'][f] == [0.0, 0.0, 1.0]).all() and (rooms[r]['curvatures'][f] == 1.0 / 6.0).all()
            assert (rooms[r]['normal_slack'][f] == 0).all() and (rooms[r]['curv_slack'][f] == 0).all()


def test_lapack_route_unchanged(B, lap, ver, lap_labels, cuda_device):
    golden = np.load(os.path.join(GOLDEN, 'baselines_ref_cpu.npz'))
    for mode in MODES:
        for r in ROOMS:
            assert np.array_equal(lap_labels[mode][r], golden['%s__label%d' % (mode, r)]), (mode, r)
    labels, counts, stats = B.segment(lap, 'feature', device=cuda_device, return_counts=True, return_stats=True)
    assert stats is None
    assert all(np.array_equal(a, b) for a, b in zip(labels, lap_labels['feature']))
    assert [int(c) for c in counts] == [int(l.max()) for l in labels]
    labels, stats = B.segment(lap, 'normal', device=cuda_device, return_stats=True)
    assert stats is None and all(np.array_equal(a, b) for a, b in zip(labels, lap_labels['normal']))
    # one room without slacks in the batch: the whole call takes the old path
    mixed = [copy.deepcopy(ver[0]), lap[1]]
    assert B.segment(mixed, 'normal', device=cuda_device, return_stats=True)[1] is None
    assert np.array_equal(mixed[0]['normals'].view(np.uint64), ver[0]['normals'].view(np.uint64))
    with pytest.raises(ValueError):
        B.room_features(np.zeros((4, 6), np.float32), device=cuda_device, eig='jacobi')


def test_redo_stays_small(B, ver, cuda_device):
    for mode in MODES:
        _, stats = B.segment(copy.deepcopy(ver), mode, device=cuda_device, return_stats=True)
        for r in ROOMS:
            n = len(ver[r]['points'])
            print('%s room %d: the edge certificate flags %d of %d points' % (mode, r, stats['flagged'][r], n))
            assert stats['flagged'][r] <= 0.01 * n, (mode, r, stats['flagged'][r], n)
    for r in ROOMS:
        s = ver[r]['verify_stats']
        share = s['rank_redone'] / s['points']
        print('room %d: rank step redoes %d of %d points (%.1f %%), %d without a bound' % (r, s['rank_redone'], s['points'], 100 * share, s['degenerate']))
        if r != 2:                                                  # the sparse-patch room is full of tied curvatures: exempt
            assert share <= 0.15, (r, share)
