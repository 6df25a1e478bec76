"""CPU: the NumPy restatement of tf_ops/sampling and tf_ops/3d_interpolation (tests/sampling_ref.py) against the reference's
own CPU functions (tests/golden/interpolate_ref_cpu.npz) and known answers, and the C-ABI entry points of the port."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
import sampling_ref as R

CASES = ('random', 'grid_ties', 'duplicates', 'm1', 'm2', 'random_int')


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'interpolate_ref_cpu.npz'))


@pytest.mark.parametrize('case', CASES)
def test_restatement_equals_reference_cpu(golden, case):
    g = {k.split('__')[1]: golden[k] for k in golden.files if k.startswith(case + '__')}
    dist, idx = R.three_nn(g['xyz1'], g['xyz2'])
    assert np.array_equal(idx, g['idx'])
    assert np.array_equal(dist.view(np.uint32), g['dist'].view(np.uint32))
    out = R.three_interpolate(g['points'], g['idx'], g['weight'])
    assert np.array_equal(out.view(np.uint32), g['out'].view(np.uint32))
    gp = R.three_interpolate_grad(g['points'].shape[1], g['idx'], g['weight'], g['grad_out'])
    assert np.array_equal(gp.view(np.uint32), g['grad_points'].view(np.uint32))


def test_golden_covers_ties_and_missing_neighbours(golden):
    # the grid case has queries with several known points at the same distance, the m < 3 cases keep (inf, 0)
    x1, x2 = golden['grid_ties__xyz1'], golden['grid_ties__xyz2']
    d = R.sqdist(x1[0][:, None, :], x2[0][None, :, :])
    assert (np.sort(d, axis=1)[:, 1] == np.sort(d, axis=1)[:, 2]).any()
    for case, m in (('m1', 1), ('m2', 2)):
        assert np.isinf(golden[case + '__dist'][:, :, m:]).all() and (golden[case + '__idx'][:, :, m:] == 0).all()


def test_fps_collinear():
    x = np.zeros((1, 9, 3), np.float32)
    x[0, :, 0] = np.arange(9)
    # 0, the far end, the middle, then the quarter points (1 before 3 among equals: the tie rule), then the rest
    assert R.farthest_point_sample(5, x)[0].tolist() == [0, 8, 4, 2, 6]


def test_fps_duplicates_and_more_samples_than_points():
    x = np.array([[[0, 0, 0], [0, 0, 0], [1, 0, 0], [1, 0, 0]]], np.float32)
    assert R.farthest_point_sample(6, x)[0].tolist() == [0, 2, 0, 0, 0, 0]
    # m > n: every point once, then index 0 repeats once every running minimum is 0
    rs = np.random.RandomState(1)
    y = rs.rand(2, 7, 3).astype(np.float32)
    out = R.farthest_point_sample(12, y)
    for row in out:
        assert sorted(row[:7].tolist()) == list(range(7)) and (row[7:] == 0).all()


def test_fps_tie_rule_is_k_mod_512_first():
    # 1030 copies of one point after point 0 sit at one distance: the reference's 512-thread scan picks the smallest (k mod 512, k)
    x = np.zeros((1, 1030, 3), np.float32)
    x[0, 1:] = 1.0
    assert R.farthest_point_sample(3, x)[0].tolist() == [0, 512, 0]
    x[0, 512] = 0.0
    assert R.farthest_point_sample(3, x)[0].tolist() == [0, 1024, 0]


def test_prob_sample_known_answer():
    inp = np.array([[1, 0, 2, 1]], np.float32)
    r = np.array([[0.0, 0.2, 0.25, 0.5, 0.75, 0.99]], np.float32)
    assert R.prob_sample(inp, r).tolist() == [[0, 0, 0, 2, 2, 3]]


def test_fp_weights():
    w = R.fp_weights(np.array([[[1, 1, 2], [0, 4, np.inf]]], np.float32))
    assert np.allclose(w[0, 0], [0.4, 0.4, 0.2]) and w[0, 1, 0] == 1.0 and w[0, 1, 2] == 0.0


NEW_SYMBOLS = ('lrg_farthest_point_sample', 'lrg_gather_point', 'lrg_scatter_add_point', 'lrg_prob_sample', 'lrg_three_nn',
               'lrg_three_interpolate', 'lrg_three_interpolate_grad', 'lrg_three_nn_interpolate')


def test_library_exports_sampling_and_interpolation(hip_lib):
    from learn_region_grow_amd import _lib
    for name in NEW_SYMBOLS:
        assert hasattr(hip_lib, name), name
        assert name in _lib.EXPORTS
    import learn_region_grow_amd.interpolate  # noqa: F401
    import learn_region_grow_amd.sampling  # noqa: F401


def test_bad_sizes_are_rejected_without_a_gpu(hip_lib):
    # argument checks run on the host before any launch (LRG_EINVAL = -1000 - n)
    assert hip_lib.lrg_farthest_point_sample(-1, 4, 4, None, None, None, None) <= -1000
    assert hip_lib.lrg_farthest_point_sample(2, 0, 4, None, None, None, None) <= -1000
    assert hip_lib.lrg_farthest_point_sample(2, 4, 0, None, None, None, None) == 0          # m <= 0 writes nothing
    assert hip_lib.lrg_three_nn(1, -3, 2, None, None, None, None, None) <= -1000
    assert hip_lib.lrg_three_nn_interpolate(1, 4, 0, 2, None, None, None, None, None, None, None, None) <= -1000
    assert hip_lib.lrg_prob_sample(1, 0, 3, None, None, None, None, None) <= -1000
    assert hip_lib.lrg_three_interpolate(1, 2, -1, 4, None, None, None, None, None) <= -1000
