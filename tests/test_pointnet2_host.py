"""CPU: the host side of the PointNet2 baseline -- the checkpoint's variable table and loader, the cells and padded inputs of
benchmarks.py:281-298 against tests/pointnet2_ref.py, and the command line's options.

tests/golden/pointnet2_model5_names.json holds the variable names and shapes of the reference's shipped
models/pointnet2_model5.ckpt.index (data only; the weights themselves are not shipped).  It was written by

    python -c "import json; from learn_region_grow_amd import checkpoint; \\
        _, e = checkpoint.read_bundle_index('<reference>/models/pointnet2_model5.ckpt'); \\
        print(json.dumps({n: list(x.shape) for n, x in sorted(e.items())}))"

and reformatted to one variable per line.
"""
import json
import os

import numpy as np
import pytest

import pointnet2_ref as R
from conftest import GOLDEN, REPO
from learn_region_grow_amd import checkpoint
from learn_region_grow_amd import pointnet2 as P


def shipped_names():
    return {k: tuple(v) for k, v in json.load(open(os.path.join(GOLDEN, 'pointnet2_model5_names.json'))).items()}


def test_shapes_equal_the_shipped_index():
    shipped = shipped_names()
    trainable = {k: v for k, v in shipped.items() if not k.endswith('/Adam') and not k.endswith('/Adam_1')
                 and k not in ('Variable', 'beta1_power', 'beta2_power')}
    ours = {k: tuple(v) for k, v in checkpoint.pointnet2_variable_shapes(13, rgb_features=False).items()}
    assert ours == trainable
    assert len(ours) == 46
    assert checkpoint.pointnet2_variant(shipped) == (13, False)
    # the restatement states the table independently, in both variants and at every class count of the reference's data sets
    for nc in (13, 40, 260):
        for rgb in (False, True):
            assert {k: tuple(v) for k, v in checkpoint.pointnet2_variable_shapes(nc, rgb).items()} == R.variable_shapes(nc, rgb)
    rgb = checkpoint.pointnet2_variable_shapes(13, True)
    assert rgb['layer1/kernel0'] == (1, 1, 6, 32) and rgb['fa_layer4/kernel0'] == (1, 1, 131, 128)


def _bundle(weights, step=7):
    out = dict(weights)
    for k, w in weights.items():                                     # what Saver().save writes besides: ignored by the loader
        out[k + '/Adam'] = np.zeros_like(w)
        out[k + '/Adam_1'] = np.ones_like(w)
    out['beta1_power'] = np.float32(0.9)
    out['beta2_power'] = np.float32(0.999)
    out['Variable'] = np.int32(step)
    return out


@pytest.mark.parametrize('num_class,rgb', [(13, False), (260, True)])
def test_bundle_round_trip_bit_for_bit(tmp_path, num_class, rgb):
    w = R.random_weights(3, num_class, rgb)
    prefix = str(tmp_path / 'pn2.ckpt')
    checkpoint.write_bundle(prefix, _bundle(w))
    got = checkpoint.load_pointnet2_weights(prefix)
    assert sorted(got) == sorted(w)
    for k in w:
        assert got[k].dtype == np.float32 and got[k].shape == w[k].shape
        assert got[k].tobytes() == w[k].tobytes(), k


def test_loader_names_what_is_wrong(tmp_path):
    w = R.random_weights(4, 13, False)
    prefix = str(tmp_path / 'bad.ckpt')
    missing = {k: v for k, v in w.items() if k != 'fa_layer2/bias1'}
    checkpoint.write_bundle(prefix, _bundle(missing))
    with pytest.raises(checkpoint.BundleError, match='fa_layer2/bias1'):
        checkpoint.load_pointnet2_weights(prefix)
    shaped = dict(w)
    shaped['layer3/kernel1'] = np.zeros((1, 1, 128, 96), np.float32)
    checkpoint.write_bundle(prefix, _bundle(shaped))
    with pytest.raises(checkpoint.BundleError, match='layer3/kernel1'):
        checkpoint.load_pointnet2_weights(prefix)
    mixed = dict(w)                                                  # colour at layer1 but not at fa_layer4
    mixed['layer1/kernel0'] = np.zeros((1, 1, 6, 32), np.float32)
    checkpoint.write_bundle(prefix, _bundle(mixed))
    with pytest.raises(checkpoint.BundleError, match='disagree'):
        checkpoint.load_pointnet2_weights(prefix)
    nohead = {k: v for k, v in w.items() if k != 'kernel2'}
    checkpoint.write_bundle(prefix, _bundle(nohead))
    with pytest.raises(checkpoint.BundleError, match='kernel2'):
        checkpoint.load_pointnet2_weights(prefix)


def _room(seed=0):
    """Points with the cases of the cell cut: negative coordinates, coordinates exactly at a half-cell (round half to even), a
    cell of one point, a cell of exactly 1024 points."""
    rng = np.random.RandomState(seed)
    parts = [rng.uniform(-2.2, 2.4, (700, 6)),
             np.array([[0.5, 0.5, 1.0, 0, 0, 0], [1.5, -0.5, 0.2, 0, 0, 0], [-1.5, 2.5, 0.3, 0, 0, 0], [-0.5, -2.5, 0.1, 0, 0, 0]]),
             np.concatenate([[[7.2, 7.3]], rng.uniform(0, 1, (1, 4))], axis=1),                       # alone in cell (7, 7)
             np.concatenate([rng.uniform(-0.45, 0.45, (1024, 2)) + [20, -20], rng.uniform(0, 3, (1024, 4))], axis=1)]
    p = np.concatenate(parts).astype(np.float32)
    return p[rng.permutation(len(p))]


@pytest.mark.parametrize('res', [1.0, 3.0])
def test_cells_and_inputs_equal_the_restatement(res):
    p = _room()
    want_members = R.cells(p, res)
    want_inputs = R.cell_inputs(p, res)
    keys, members = P.cells(p, res)
    assert sorted(map(tuple, keys.tolist())) == sorted(want_members)
    batch, members2, keys2 = P.cell_inputs(p, res, room='r0')
    assert batch.dtype == np.float32 and batch.shape == (len(keys), 1024, 6)
    assert np.array_equal(keys, keys2)
    for c, k in enumerate(map(tuple, keys.tolist())):
        assert np.array_equal(members[c], want_members[k]) and np.array_equal(members2[c], want_members[k])
        assert batch[c].tobytes() == want_inputs[k].tobytes(), k
    if res == 1.0:
        sizes = {tuple(k): len(m) for k, m in zip(keys.tolist(), members)}
        assert sizes[(7, 7)] == 1 and sizes[(20, -20)] == 1024
        # half to even: 0.5 -> 0, 1.5 -> 2, -0.5 -> -0, -1.5 -> -2, 2.5 -> 2, -2.5 -> -2
        half = {(0, 0), (2, 0), (-2, 2), (0, -2)}
        got = set(map(tuple, np.round(np.array([[0.5, 0.5], [1.5, -0.5], [-1.5, 2.5], [-0.5, -2.5]], np.float32)).astype(int).tolist()))
        assert got == half and half <= set(sizes)
        one = batch[[tuple(k) for k in keys.tolist()].index((7, 7))]
        assert (one == one[0]).all() and one[0, 2] == 0                # a single point: 1024 copies, z minus its own minimum


def test_a_cell_of_1025_points_is_a_value_error():
    rng = np.random.RandomState(1)
    p = np.concatenate([rng.uniform(-0.4, 0.4, (1025, 2)) + [3, -4], rng.uniform(0, 1, (1025, 4))], axis=1).astype(np.float32)
    with pytest.raises(ValueError, match=r'room kitchen_2.*\(3, -4\).*1025'):
        P.cell_inputs(p, 1.0, room='kitchen_2')
    with pytest.raises(ValueError):
        R.cell_inputs(p, 1.0)
    P.cell_inputs(p[:1024], 1.0)


def test_grid_resolution_follows_the_area_name():
    assert P.grid_resolution('kitti_val') == 3.0 and P.grid_resolution('kitti_small') == 3.0
    assert P.grid_resolution('5') == 1.0 and P.grid_resolution('scannet') == 1.0 and P.grid_resolution(5) == 1.0
    p = _room()
    keys3, _ = P.cells(p, P.grid_resolution('kitti_train'))
    assert sorted(map(tuple, keys3.tolist())) == sorted(R.cells(p, 3.0))


def test_cli_parse():
    import importlib.util
    spec = importlib.util.spec_from_file_location('pointnet2_cli', os.path.join(REPO, 'pointnet2.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.parse([])
    assert (a.area, a.h5, a.ckpt, a.save, a.room_names, a.max_rooms, a.batch_rooms, a.device, a.metrics) == \
        ('1,2,3,4,5,6,scannet', None, None, None, None, 0, 68, None, 'host')
    assert cli.model_path(a, '3') == 'models/pointnet2_model3.ckpt' and cli.model_path(a, 'scannet') == 'models/pointnet2_model5.ckpt'
    a = cli.parse(['--h5', 'x.h5', '--area', 'kitti_val', '--ckpt', 'm.ckpt', '--save', '--room-names', 'n.txt', '--max-rooms', '2',
                   '--batch-rooms', '4', '--device', 'cuda:1', '--metrics', 'device'])
    assert (a.area, a.h5, a.ckpt, a.save, a.room_names, a.max_rooms, a.batch_rooms, a.device, a.metrics) == \
        ('kitti_val', 'x.h5', 'm.ckpt', '', 'n.txt', 2, 4, 'cuda:1', 'device')
    assert cli.model_path(a, 'kitti_val') == 'm.ckpt'
    assert cli.parse(['--save', 'out']).save == 'out'
    with pytest.raises(SystemExit):
        cli.parse(['--metrics', 'nowhere'])
