"""CPU: the twin of the device batch assembly (tests/assemble_ref.py) has the properties the kernel is held to, the binding declares
the two entry points of ABI 24, and train_region_grow.py's parser knows the device path's switches.  No GPU."""
import numpy as np
import pytest

import assemble_ref

K = 64


@pytest.mark.parametrize('N', [64, 65, 129, 1024, 3000])
def test_subset_positions_are_distinct_and_in_range(N):
    for purpose in (assemble_ref.TRAIN_INLIER, assemble_ref.TRAIN_NEIGHBOR):
        p = assemble_ref.positions(7, 3, N, K, purpose, 0, 0)
        assert p.shape == (K,) and p.min() >= 0 and p.max() < N
        assert len(set(p.tolist())) == K


@pytest.mark.parametrize('N', [1, 2, 63])
def test_padded_positions_lead_with_every_row(N):
    p = assemble_ref.positions(7, 3, N, K, assemble_ref.TRAIN_INLIER, 0, 0)
    assert p[:N].tolist() == list(range(N))
    assert p.shape == (K,) and p[N:].min() >= 0 and p[N:].max() < N


def test_epoch_pass_and_tuple_id_each_change_the_draws():
    base = assemble_ref.positions(7, 3, 3000, K, assemble_ref.TRAIN_INLIER, 0, 0).tolist()
    assert base == assemble_ref.positions(7, 3, 3000, K, assemble_ref.TRAIN_INLIER, 0, 0).tolist()
    assert base != assemble_ref.positions(7, 3, 3000, K, assemble_ref.TRAIN_INLIER, 1, 0).tolist()      # another epoch
    assert base != assemble_ref.positions(7, 3, 3000, K, assemble_ref.TRAIN_INLIER, 0, 1).tolist()      # another pass
    assert base != assemble_ref.positions(7, 4, 3000, K, assemble_ref.TRAIN_INLIER, 0, 0).tolist()      # another tuple
    assert base != assemble_ref.positions(8, 3, 3000, K, assemble_ref.TRAIN_INLIER, 0, 0).tolist()      # another seed
    assert base != assemble_ref.positions(7, 3, 3000, K, assemble_ref.TRAIN_NEIGHBOR, 0, 0).tolist()    # the other side


def test_twin_batch_does_not_depend_on_the_batch_position():
    tup = assemble_ref.constructed_tuples()
    a = assemble_ref.assemble_batch(tup, [6, 1, 7], K, K, 13, 5, 2, 0)
    b = assemble_ref.assemble_batch(tup, [7, 6], K, K, 13, 5, 2, 0)
    for x, y in zip(a, b):
        assert np.array_equal(x[0], y[1]) and np.array_equal(x[2], y[0])
    xi, xn, ia, ir, pr, pa = a
    assert xi.shape == (3, K, 13) and ia.shape == (3, K) and pr.tolist() == ir.sum(axis=1).tolist() and pa.tolist() == ia.sum(axis=1).tolist()
    # every gathered row is a row of its tuple, flag and all
    for b_, t in enumerate([6, 1, 7]):
        at = (xi[b_, :, 0] / 13).astype(np.int64)
        assert at.min() >= tup['start_in'][t] and at.max() < tup['start_in'][t] + tup['count_in'][t]
        assert np.array_equal(tup['points'][at], xi[b_]) and np.array_equal(tup['remove'][at], ir[b_])


def test_binding_declares_the_entry_points():
    from learn_region_grow_amd import _lib
    assert 'lrg_train_assemble' in _lib.EXPORTS and 'lrg_ce_grad_counted' in _lib.EXPORTS
    assert 'lrg_assemble.hip' in _lib.SOURCES and _lib.LRG_ABI_VERSION >= 24
    assert (_lib.LRG_PURPOSE_TRAIN_INLIER, _lib.LRG_PURPOSE_TRAIN_NEIGHBOR) == (assemble_ref.TRAIN_INLIER, assemble_ref.TRAIN_NEIGHBOR)


def test_parser_knows_the_device_path():
    import train_region_grow
    args = train_region_grow.parse([])
    assert (args.assemble, args.stage) == ('host', 'files')                          # the default stays the host path on staged files
    assert train_region_grow.parse(['--assemble', 'device']).assemble == 'device'
    args = train_region_grow.parse(['--stage', 'online', '--max-points', '512', '--resolution', '0.2'])
    assert (args.assemble, args.stage, args.max_points, args.resolution) == ('device', 'online', 512, 0.2)
    assert train_region_grow.parse(['--stage', 'online', '--assemble', 'device']).assemble == 'device'
    with pytest.raises(SystemExit):
        train_region_grow.parse(['--stage', 'online', '--assemble', 'host'])
