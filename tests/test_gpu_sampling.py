"""GPU: tf_ops/sampling and tf_ops/3d_interpolation replacements against the NumPy restatement (tests/sampling_ref.py), which
equals the reference's own CPU functions (tests/test_sampling_oracle.py), and against the golden inputs and outputs."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
import sampling_ref as R

pytestmark = pytest.mark.gpu


def dev(a, cuda_device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda_device)


def host(t):
    return t.cpu().numpy()


def bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), 'max |diff| %g' % np.nanmax(np.abs(a.astype(np.float64) - b))


def fps_points(b, n, seed):
    """Half the batch on a coarse grid (many equal distances and duplicated points), half uniform."""
    rs = np.random.RandomState(seed)
    x = rs.rand(b, n, 3).astype(np.float32)
    x[: (b + 1) // 2] = np.floor(x[: (b + 1) // 2] * 6).astype(np.float32)
    return x


# b in {1, 3, 100}; n across the register buckets (1024 | 4096 | 8192 | 16384 points) and the streaming path; m > n
@pytest.mark.parametrize('b,n,m', [(1, 64, 100), (3, 1000, 300), (100, 1024, 256), (3, 1025, 40), (3, 4096, 40), (3, 4097, 40),
                                   (1, 8193, 40), (1, 16384, 40), (1, 16385, 40), (1, 32768, 128), (1, 131072, 64)])
def test_fps_equals_restatement(cuda_device, b, n, m):
    from learn_region_grow_amd import sampling
    x = fps_points(b, n, n + b)
    got = host(sampling.farthest_point_sample(m, dev(x, cuda_device)))
    np.testing.assert_array_equal(got, R.farthest_point_sample(m, x))


def test_fps_tie_rule_and_repeats(cuda_device):
    from learn_region_grow_amd import sampling
    x = np.zeros((2, 1030, 3), np.float32)
    x[:, 1:] = 1.0
    x[1, 512] = 0.0
    got = host(sampling.farthest_point_sample(4, dev(x, cuda_device)))
    assert got.tolist() == [[0, 512, 0, 0], [0, 1024, 0, 0]]
    # all points equal, streaming path: index 0 throughout
    y = np.ones((1, 20000, 3), np.float32)
    assert (host(sampling.farthest_point_sample(5, dev(y, cuda_device))) == 0).all()
    with pytest.raises(ValueError):
        sampling.farthest_point_sample(0, dev(x, cuda_device))


def test_gather_point_and_grad(cuda_device):
    from learn_region_grow_amd import sampling
    rs = np.random.RandomState(3)
    inp = rs.randn(3, 500, 3).astype(np.float32)
    idx = rs.randint(0, 500, (3, 800)).astype(np.int32)              # repeated indices: colliding atomics
    out = sampling.gather_point(dev(inp, cuda_device), dev(idx, cuda_device))
    bits_equal(host(out), R.gather_point(inp, idx))
    gi = rs.randint(-8, 9, (3, 800, 3)).astype(np.float32)           # integer values: exact in any order
    g = sampling.gather_point_grad(dev(inp, cuda_device), dev(idx, cuda_device), dev(gi, cuda_device))
    bits_equal(host(g), R.gather_point_grad(500, idx, gi))
    gr = rs.randn(3, 800, 3).astype(np.float32)
    g = sampling.gather_point_grad(dev(inp, cuda_device), dev(idx, cuda_device), dev(gr, cuda_device))
    np.testing.assert_allclose(host(g), R.gather_point_grad(500, idx, gr), rtol=1e-5, atol=1e-5)
    with pytest.raises(ValueError):
        sampling.gather_point(dev(inp[:, :, :2], cuda_device), dev(idx, cuda_device))
    with pytest.raises(ValueError):
        sampling.gather_point_grad(dev(inp, cuda_device), dev(idx, cuda_device), dev(gr[:, :5], cuda_device))


def test_prob_sample(cuda_device):
    from learn_region_grow_amd import sampling
    rs = np.random.RandomState(4)
    # integer-valued weights: the cdf is exact in any summation order, so the indices equal the restatement's
    w = rs.randint(0, 5, (4, 3000)).astype(np.float32)
    r = rs.rand(4, 700).astype(np.float32)
    np.testing.assert_array_equal(host(sampling.prob_sample(dev(w, cuda_device), dev(r, cuda_device))), R.prob_sample(w, r))
    # random weights: every index brackets its query by the float64 cdf, except within n eps of a boundary
    w = rs.rand(3, 5000).astype(np.float32)
    r = rs.rand(3, 900).astype(np.float32)
    got = host(sampling.prob_sample(dev(w, cuda_device), dev(r, cuda_device))).astype(np.int64)
    cdf = np.cumsum(w.astype(np.float64), axis=1)
    q = r.astype(np.float64) * cdf[:, -1:]
    rows = np.arange(3)[:, None]
    hi = cdf[rows, got]
    lo = np.where(got > 0, cdf[rows, np.maximum(got - 1, 0)], -np.inf)
    tol = 5000 * np.finfo(np.float32).eps * cdf[:, -1:]
    assert ((lo < q + tol) & (q <= hi + tol)).all()
    with pytest.raises(ValueError):
        sampling.prob_sample(dev(w, cuda_device), dev(r[:2], cuda_device))


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'interpolate_ref_cpu.npz'))


@pytest.mark.parametrize('case', ('random', 'grid_ties', 'duplicates', 'm1', 'm2', 'random_int'))
def test_interpolate_golden(cuda_device, golden, case):
    from learn_region_grow_amd import interpolate
    g = {k.split('__')[1]: golden[k] for k in golden.files if k.startswith(case + '__')}
    dist, idx = interpolate.three_nn(dev(g['xyz1'], cuda_device), dev(g['xyz2'], cuda_device))
    np.testing.assert_array_equal(host(idx), g['idx'])
    bits_equal(host(dist), g['dist'])
    out = interpolate.three_interpolate(dev(g['points'], cuda_device), dev(g['idx'], cuda_device), dev(g['weight'], cuda_device))
    bits_equal(host(out), g['out'])
    gp = interpolate.three_interpolate_grad(dev(g['points'], cuda_device), dev(g['idx'], cuda_device), dev(g['weight'], cuda_device),
                                            dev(g['grad_out'], cuda_device))
    if case.endswith('int') or case in ('grid_ties', 'duplicates', 'm1', 'm2'):
        bits_equal(host(gp), g['grad_points'])                          # integer-valued inputs: exact in any atomic order
    else:
        np.testing.assert_allclose(host(gp), g['grad_points'], rtol=1e-5, atol=1e-5)


# the PointNet2 shapes (b = 100 there; fewer here to keep the NumPy side quick) plus tiles of known points beyond one LDS tile
@pytest.mark.parametrize('b,n,m,c', [(4, 64, 16, 512), (4, 256, 64, 128), (2, 1024, 256, 128), (1, 1024, 1024, 128), (2, 300, 2500, 5),
                                     (2, 100, 2, 3), (1, 257, 1, 1)])
def test_three_nn_interpolate_equals_restatement(cuda_device, b, n, m, c):
    from learn_region_grow_amd import interpolate
    rs = np.random.RandomState(n + m)
    x1 = rs.rand(b, n, 3).astype(np.float32)
    x2 = rs.rand(b, m, 3).astype(np.float32)
    x2[:, m // 2:] = np.floor(x2[:, m // 2:] * 4) / 4           # duplicated known points: equal distances
    x1[:, : n // 3] = x2[:, rs.randint(0, m, n // 3)]           # queries ON known points: d = 0, the 1e-10 clamp
    pts = rs.randn(b, m, c).astype(np.float32)
    wd, wi = R.three_nn(x1, x2)
    d1, d2, dp = dev(x1, cuda_device), dev(x2, cuda_device), dev(pts, cuda_device)
    dist, idx = interpolate.three_nn(d1, d2)
    np.testing.assert_array_equal(host(idx), wi)
    bits_equal(host(dist), wd)
    w = R.fp_weights(wd)
    out = interpolate.three_interpolate(dp, idx, dev(w, cuda_device))
    bits_equal(host(out), R.three_interpolate(pts, wi, w))
    # the fused launch equals the unfused chain with the weights computed in NumPy float32
    fused, fw = interpolate.three_nn_interpolate(d1, d2, dp, return_weight=True)
    bits_equal(host(fw), w)
    bits_equal(host(fused), host(out))
    bits_equal(host(interpolate.three_nn_interpolate(d1, d2, dp)), host(out))
    go = rs.randint(-4, 5, (b, n, c)).astype(np.float32)
    wi_int = rs.randint(-2, 3, (b, n, 3)).astype(np.float32)
    gp = interpolate.three_interpolate_grad(dp, idx, dev(wi_int, cuda_device), dev(go, cuda_device))
    bits_equal(host(gp), R.three_interpolate_grad(m, wi, wi_int, go))


def test_interpolate_shape_errors(cuda_device):
    from learn_region_grow_amd import interpolate
    x = dev(np.zeros((2, 10, 3), np.float32), cuda_device)
    with pytest.raises(ValueError):
        interpolate.three_nn(x, dev(np.zeros((3, 4, 3), np.float32), cuda_device))
    with pytest.raises(ValueError):
        interpolate.three_nn(dev(np.zeros((2, 10, 2), np.float32), cuda_device), x)
    with pytest.raises(ValueError):
        interpolate.three_interpolate(x, dev(np.zeros((2, 10, 2), np.int32), cuda_device), x)
    with pytest.raises(ValueError):
        interpolate.three_nn_interpolate(x, dev(np.zeros((2, 0, 3), np.float32), cuda_device), dev(np.zeros((2, 0, 4), np.float32), cuda_device))


def test_sample_and_group_equals_composition(cuda_device):
    from learn_region_grow_amd import grouping, sampling
    rs = np.random.RandomState(5)
    xyz = dev(rs.rand(4, 1024, 3).astype(np.float32), cuda_device)
    pts = dev(rs.randn(4, 1024, 6).astype(np.float32), cuda_device)
    new_xyz, new_points, idx, gx = grouping.sample_and_group(256, 0.2, 32, xyz, pts)
    fi = sampling.farthest_point_sample(256, xyz)
    want_xyz = sampling.gather_point(xyz, fi)
    bits_equal(host(new_xyz), R.gather_point(host(xyz), host(fi)))
    bits_equal(host(new_xyz), host(want_xyz))
    widx, _ = grouping.query_ball_point(0.2, 32, xyz, want_xyz)
    np.testing.assert_array_equal(host(idx), host(widx))
    wgx = host(grouping.group_point(xyz, widx)) - host(want_xyz)[:, :, None, :]
    bits_equal(host(gx), wgx)
    bits_equal(host(new_points), np.concatenate([wgx, host(grouping.group_point(pts, widx))], -1))
    _, np_only, _, gx2 = grouping.sample_and_group(256, 0.2, 32, xyz, None)
    bits_equal(host(np_only), host(gx2))
