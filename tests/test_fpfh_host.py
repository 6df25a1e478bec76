"""CPU: the FPFH mode's definition as tests/fpfh_ref.py states it, and its plumbing: how many points of the fixture
rooms the near rule excuses, the +-2 voxel window against a scan of all pairs, the PCD round trip, two rooms whose histograms are
known in closed form."""
import os
import re

import numpy as np
import pytest

from conftest import REPO
import baselines_ref as R
import fpfh_ref as F


@pytest.fixture(scope='module')
def feats():
    return [R.features(raw) for raw in R.golden_rooms()]


@pytest.fixture(scope='module')
def twins(feats):
    return [F.twin(f) for f in feats]


def test_excused_points_are_few(twins):
    """The near rule (DELTA = 1e-4) excuses at most 8 % of every fixture room (measured: 4.6 %, 3.6 %, 5.9 %), and float32 and
    float64 pair features agree on every bin of every pair that is not near."""
    for r, t in enumerate(twins):
        share = t['excused'].mean()
        disagree = (t['bins32'] != t['bins64']).any(axis=1) | (t['ok32'] != t['ok64'])
        print('room %d: %d points, %d pairs, excused %.2f %%, float32/float64 disagreements %d' % (r, t['N'], len(t['I']), 100 * share, disagree.sum()))
        assert share <= 0.08, (r, share)
        assert not (disagree & ~t['near']).any(), r
        assert np.array_equal(t['counts32'][~t['excused']], t['counts64'][~t['excused']])


def test_window_loses_no_pair_of_the_ball(feats, twins):
    """Every pair with d2 <= r2 lies in the +-2 voxel window: the per-point count over ALL points equals k.  The scan knows nothing
    of voxels; it only leaves out the points further than 0.25 away in x, whose d2 is above 0.06 > r2."""
    r2 = np.float32(0.2) * np.float32(0.2)
    for f, t in zip(feats, twins):
        order = np.argsort(t['P'][:, 0], kind='stable')
        P = t['P'][order]
        k = np.zeros(len(P), dtype=np.int64)
        for c0 in range(0, len(P), 512):
            c1 = min(len(P), c0 + 512)
            lo, hi = np.searchsorted(P[:, 0], P[c0, 0] - 0.25), np.searchsorted(P[:, 0], P[c1 - 1, 0] + 0.25, side='right')
            d = P[None, lo:hi, :] - P[c0:c1, None, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            k[c0:c1] = (d2 <= r2).sum(axis=1)
        assert np.array_equal(k, t['k'][order])


def test_pcd_roundtrip_equals_string_route(feats):
    from learn_region_grow_amd import baselines
    for f in feats:
        for a in (f['points'][:, :3], f['normals'].astype(np.float32)):
            assert np.array_equal(baselines.pcd_roundtrip(a).view(np.uint32), F.roundtrip_str(a).view(np.uint32))
    # ties of the sixth decimal (exact in float32), signed zeros, large and tiny values
    a = np.array([0.5 ** 7, 3 * 0.5 ** 7, -0.5 ** 7, 0.0, -0.0, -1e-8, 1e-8, 123456.789, -98765.4321, 1e9, 2.5e-7, 1.5e-6, 0.1, 1 / 3], np.float32)
    got = baselines.pcd_roundtrip(a)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), F.roundtrip_str(a).view(np.uint32))
    assert baselines.pcd_roundtrip(a.reshape(7, 2)).shape == (7, 2)


def test_flat_patch_is_exact():
    room = F.flat_patch()
    t = F.twin(room)
    assert t['k'].min() >= 4
    want = np.zeros(33, np.float32)
    want[[5, 16, 27]] = 100.0
    h = F.describe(room)
    assert h.dtype == np.float32 and (h == want[None, :]).all()
    for g in range(3):
        assert (t['counts32'][:, 11 * g:11 * g + 11].sum(axis=1) == t['k'] - 1).all()


def test_one_point_room_has_no_histogram_and_no_edge():
    room = F.make_room([[0.3, 0.2, 0.1]])
    t = F.twin(room)
    assert t['k'].tolist() == [1] and not t['counts32'].any()
    h = F.describe(room)
    assert h.shape == (1, 33) and not h.any()
    assert np.isnan(F.unit(h)).all()
    two = F.make_room([[0, 0, 0], [0.1, 0, 0]])
    assert not F.edge(F.unit(np.zeros((2, 33), np.float32)), np.array([1]), np.array([0]), -1.0).any()
    assert F.segment(two['points'], np.zeros((2, 33), np.float32), -1.0, min_cluster_size=1).tolist() == [0, 0]


def test_plumbing():
    from learn_region_grow_amd import _lib, baselines
    assert baselines.MODES == ('normal', 'curvature', 'color', 'feature', 'smoothness')
    assert baselines.ALL_MODES == baselines.MODES + ('fpfh',)
    assert baselines.default_thresholds('fpfh') == (0.985, 0.0, 0.0)
    assert baselines.default_thresholds('fpfh', 'scannet') == (0.985, 0.0, 0.0)
    with pytest.raises(ValueError):
        baselines.default_thresholds('edge')
    for name in ('lrg_fpfh_workspace_bytes', 'lrg_fpfh', 'lrg_fpfh_status', 'lrg_baseline_fpfh_workspace_bytes', 'lrg_baseline_segment_fpfh'):
        assert name in _lib.EXPORTS
    assert 'lrg_fpfh.hip' in _lib.SOURCES and os.path.exists(os.path.join(_lib.CSRC, 'lrg_fpfh.hip'))
    header = open(os.path.join(REPO, 'include', 'lrg_hip.h')).read()
    assert int(re.search(r'#define\s+LRG_ABI_VERSION\s+(\d+)', header).group(1)) == _lib.LRG_ABI_VERSION >= 18
    assert int(re.search(r'#define\s+LRG_FPFH_LISTS\s+(\d+)', header).group(1)) == _lib.LRG_FPFH_LISTS
    # argument checks that need no device
    with pytest.raises(ValueError, match='radius'):
        baselines.fpfh([F.flat_patch()], resolution=0.1, radius=0.25)
    with pytest.raises(ValueError, match='normals'):
        baselines.fpfh([dict(points=F.flat_patch()['points'], normals=None)])
