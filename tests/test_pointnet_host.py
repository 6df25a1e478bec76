"""CPU: the host side of the plain PointNet baseline -- the checkpoint's variable table and loader, the assumption the kernels rest
on (train_pointnet.py:57-59 subtracts the pooled row from every row), the restatement tests/pointnet_ref.py against the same
layers in torch, the batch-norm fold and the command line's options.

tests/golden/pointnet_model5_names.json holds the variable names and shapes of the reference's shipped
models/pointnet_model5.ckpt.index (data only; the weights themselves are not shipped).  It was written by

    python -c "import json; from learn_region_grow_amd import checkpoint; \\
        _, e = checkpoint.read_bundle_index('<reference>/models/pointnet_model5.ckpt'); \\
        print(json.dumps({n: list(x.shape) for n, x in sorted(e.items())}))"

and reformatted to one variable per line.
"""
import json
import os

import numpy as np
import pytest

import pointnet_ref as R
from conftest import GOLDEN, REPO
from learn_region_grow_amd import checkpoint

VARIANTS = {'shipped': R.SHIPPED + (13,), 'current': R.CURRENT + (260,)}


def shipped_names():
    return {k: tuple(v) for k, v in json.load(open(os.path.join(GOLDEN, 'pointnet_model5_names.json'))).items()}


def test_shapes_equal_the_shipped_index():
    shipped = shipped_names()
    trainable = {k: v for k, v in shipped.items() if not k.endswith('/Adam') and not k.endswith('/Adam_1')
                 and k not in ('Variable', 'beta1_power', 'beta2_power')}
    ours = {k: tuple(v) for k, v in checkpoint.pointnet_variable_shapes((64, 64, 128, 512), (512,), 13).items()}
    assert ours == trainable
    assert sorted(ours) == sorted(trainable) and len(ours) == 16
    assert checkpoint.pointnet_variant(shipped) == ((64, 64, 128, 512), (512,), 13)
    # the restatement states the table independently, for both networks and at every class count of the reference's data sets
    for conv, fc in (R.SHIPPED, R.CURRENT):
        for nc in (13, 40, 260):
            got = {k: tuple(v) for k, v in checkpoint.pointnet_variable_shapes(conv, fc, nc).items()}
            assert got == R.variable_shapes(conv, fc, nc)
            assert checkpoint.pointnet_variant(got) == (conv, fc, nc)
    assert R.variable_shapes(*VARIANTS['current'])['fc_weights0'] == (1, 1088, 512)


@pytest.mark.parametrize('name', sorted(VARIANTS))
def test_bundle_round_trip(tmp_path, name):
    conv, fc, nc = VARIANTS[name]
    w = R.random_weights(3, conv, fc, nc)
    prefix = str(tmp_path / 'ck' / 'pointnet.ckpt')
    extra = dict(w)
    extra['Variable'] = np.int32(7)
    extra['kernel0/Adam'] = np.zeros_like(w['kernel0'])               # optimizer slots are ignored
    checkpoint.write_bundle(prefix, extra)
    got = checkpoint.load_pointnet_weights(prefix)
    assert sorted(got) == sorted(w)
    for k in w:
        assert got[k].dtype == np.float32 and np.array_equal(got[k], w[k]), k


def test_second_batch_norm_block_is_found_by_its_suffix(tmp_path):
    """Block 1's moving averages under another uniquified prefix that ends in the moments suffix and contains 'bn_1/'."""
    conv, fc, nc = VARIANTS['current']
    w = R.random_weights(4, conv, fc, nc)
    other = {}
    for k, v in w.items():
        other[k.replace('bn/bn_1/', 'bn_1/bn_1/') if k.startswith('bn/bn_1/') else k] = v
    assert sorted(other) != sorted(w)
    prefix = str(tmp_path / 'pointnet.ckpt')
    checkpoint.write_bundle(prefix, other)
    got = checkpoint.load_pointnet_weights(prefix)
    for k in w:
        assert np.array_equal(got[k], w[k]), k


def _raises(tmp_path, tensors, word):
    prefix = str(tmp_path / 'bad.ckpt')
    checkpoint.write_bundle(prefix, tensors)
    with pytest.raises(checkpoint.BundleError) as e:
        checkpoint.load_pointnet_weights(prefix)
    assert word in str(e.value), str(e.value)


def test_bundle_errors_name_the_variable(tmp_path):
    conv, fc, nc = VARIANTS['current']
    good = R.random_weights(5, conv, fc, nc)
    z = lambda *s: np.zeros(s, np.float32)

    w = dict(good)
    del w['kernel1']                                                  # a missing kernel: the stack ends after kernel0
    _raises(tmp_path, w, 'kernel1')
    w = dict(good)
    del w['bias3']
    _raises(tmp_path, w, 'bias3')
    w = dict(good, fc_weights0=z(1, 1024 + 128, 512))                 # k is not conv[-1] + conv[1]
    _raises(tmp_path, w, 'fc_weights0')
    w = dict(good)
    w['bn/bn/' + R.MEAN] = z(1024, 256)                               # a moving average of the wrong shape, block 0 ...
    _raises(tmp_path, w, 'bn/bn/' + R.MEAN)
    w = dict(good)
    w['bn/bn_1/' + R.VARIANCE] = z(512, 256)                          # ... and block 1
    _raises(tmp_path, w, 'bn/bn_1/' + R.VARIANCE)
    w = dict(good)
    del w['bn/bn_1/' + R.MEAN]
    _raises(tmp_path, w, 'bn/bn_1/' + R.MEAN)
    w = dict(good, kernel2=z(1, 1, 64, 48), kernel3=z(1, 1, 48, 128))  # a width that is not a multiple of 32
    _raises(tmp_path, w, 'kernel2')
    w = dict(good, fc_weights0=z(1, 1088, 500), fc_weights1=z(1, 500, 256))
    _raises(tmp_path, w, 'fc_weights0')
    w = dict(good, kernel4=z(1, 1, 128, 2048), fc_weights0=z(1, 2048 + 64, 512))      # above the kernels' width
    _raises(tmp_path, w, 'kernel4')
    w = dict(good, fc_weights0=z(1, 1088, 1024), fc_weights1=z(1, 1024, 256))
    _raises(tmp_path, w, 'fc_weights0')
    w = dict(good, kernel2=z(1, 1, 32, 64))                           # does not continue kernel1
    _raises(tmp_path, w, 'kernel2')
    w = dict(good, fc_bias2=z(13).astype(np.float64))
    w['fc_weights2'] = z(1, 256, 13)
    _raises(tmp_path, w, 'fc_bias2')
    # the variant alone, without a file
    with pytest.raises(checkpoint.BundleError):
        checkpoint.pointnet_variant({'kernel0': (1, 6, 1, 64)})
    with pytest.raises(checkpoint.BundleError):
        checkpoint.pointnet_variant({'kernel0': (1, 3, 1, 64), 'kernel1': (1, 1, 64, 64), 'fc_weights0': (1, 128, 32), 'fc_weights1': (1, 32, 2)})
    assert checkpoint.pointnet_variant({'kernel0': (1, 6, 1, 64), 'kernel1': (1, 1, 64, 32), 'fc_weights0': (1, 64, 32),
                                        'fc_weights1': (1, 32, 1)}) == ((64, 32), (32,), 1)


def test_tile_and_reshape_subtract_the_pooled_row():
    """train_pointnet.py:56-59 at toy size (batch 2, num_point 4, 3 channels), written literally: the pool reshaped to
    [batch, 1, C], tiled num_point times along the LAST axis, reshaped to [batch, num_point, C].  Row p of the result is the
    pooled row, for every p: the assumption lrg_pointnet_head rests on."""
    rng = np.random.RandomState(0)
    batch_size, num_point, c = 2, 4, 3
    conv_last = rng.uniform(0, 1, (batch_size, num_point, 1, c))      # NHWC, W = 1
    pool = conv_last.max(axis=1, keepdims=True)                       # max_pool2d, ksize [1, num_point, 1, 1]
    tile = np.tile(pool.reshape(batch_size, -1, c), [1, 1, num_point])
    assert tile.shape == (batch_size, 1, c * num_point)
    tile = tile.reshape(batch_size, num_point, -1)
    literal = conv_last.reshape(batch_size, num_point, -1) - tile
    rows = conv_last[:, :, 0, :]
    assert np.array_equal(literal, rows - rows.max(axis=1)[:, None, :])
    assert (literal.max(axis=1) == 0).all() and (literal <= 0).all()


def _cells(seed, n_cells=2):
    rng = np.random.RandomState(seed)
    x = rng.uniform(-0.5, 0.5, (n_cells, R.NUM_POINT, 6)).astype(np.float32)
    x[:, :, 2:] = rng.uniform(0, 1, (n_cells, R.NUM_POINT, 4))
    x[1, 300:] = x[1, 0]                                              # a cell of 300 points: the padding repeats its first row
    return x


@pytest.mark.parametrize('name', sorted(VARIANTS))
def test_restatement_agrees_with_torch(name):
    """The float32 restatement against the same layers composed from torch ops on the CPU (conv1d for the 1x1 convolutions, matmul
    for the fc layers, batch_norm as tf.nn.batch_normalization orders it).  Both are float32 evaluations of the float64
    restatement with their own summation orders: torch must lie within the GPU tests' bound 8 d + 1e-6 s of the float64 values,
    d the restatement's own float32 distance."""
    import torch
    import torch.nn.functional as F
    conv, fc, nc = VARIANTS[name]
    w = R.random_weights(6, conv, fc, nc)
    x = _cells(7)
    l64, p64 = R.forward(x, w, np.float64)
    l32, p32 = R.forward(x, w, np.float32)
    assert l32.dtype == np.float32 and l64.dtype == np.float64 and l64.shape == (2, R.NUM_POINT, nc)
    with torch.no_grad():
        t = torch.from_numpy(x).permute(0, 2, 1)                      # [B, 6, 1024]
        acts = []
        for i in range(len(conv)):
            k = torch.from_numpy(w['kernel%d' % i]).reshape(-1, conv[i])                   # [cin, cout]
            t = F.relu(F.conv1d(t, k.t().unsqueeze(-1).contiguous(), torch.from_numpy(w['bias%d' % i])))
            acts.append(t)
        pooled = acts[-1].amax(dim=2, keepdim=True)
        t = torch.cat([acts[-1] - pooled, acts[1]], dim=1).permute(0, 2, 1)                # [B, 1024, conv[-1] + conv[1]]
        for j in range(len(fc)):
            t = torch.matmul(t, torch.from_numpy(w['fc_weights%d' % j][0])) + torch.from_numpy(w['fc_bias%d' % j])
            beta, gamma, mean, var = (torch.from_numpy(w[n]) for n in R.bn_names(j))
            inv = torch.rsqrt(var + 1e-3) * gamma
            t = F.relu(t * inv + (beta - mean * inv))
        t = torch.matmul(t, torch.from_numpy(w['fc_weights%d' % len(fc)][0])) + torch.from_numpy(w['fc_bias%d' % len(fc)])
    for what, got, f32, f64 in (('pooled', pooled[:, :, 0].numpy(), p32['pooled'], p64['pooled']),
                                ('skip', acts[1].permute(0, 2, 1).numpy(), p32['skip'], p64['skip']),
                                ('logits', t.numpy(), l32, l64)):
        d, s = np.abs(f32.astype(np.float64) - f64).max(), np.abs(f64).max()
        bound = 8 * d + 1e-6 * s
        err = np.abs(got.astype(np.float64) - f64).max()
        print('%s %s: d %.3e s %.3e bound %.3e torch error %.3e' % (name, what, d, s, bound, err))
        assert d > 0 and err <= bound, (what, err, bound)
    # the padding rows of the 300-point cell repeat row 0
    assert np.allclose(p64['conv'][0][1, 300:], p64['conv'][0][1, 0])


def test_fold_batch_norm_is_tensorflows_order():
    from learn_region_grow_amd import pointnet
    rng = np.random.RandomState(1)
    c = 64
    beta, gamma = rng.uniform(-0.2, 0.2, c).astype(np.float32), rng.uniform(0.5, 1.5, c).astype(np.float32)
    mean, var = rng.uniform(-0.2, 0.2, (1024, c)).astype(np.float32), rng.uniform(0.01, 0.5, (1024, c)).astype(np.float32)
    scale, shift = pointnet.fold_batch_norm(beta, gamma, mean, var)
    assert scale.dtype == shift.dtype == np.float32 and scale.shape == shift.shape == (1024, c)
    x = rng.uniform(-1, 1, (3, 1024, c)).astype(np.float32)
    assert np.array_equal(x * scale + shift, R.batch_norm(x, beta, gamma, mean, var, np.float32))
    exact = R.batch_norm(x.astype(np.float64), beta, gamma, mean, var, np.float64)
    assert np.abs(x * scale + shift - exact).max() < 1e-5
    assert scale.min() > 0.5 / np.sqrt(0.501) - 1e-3 and scale.max() < 1.5 / np.sqrt(0.011) + 1e-3


def test_cli_parse():
    import importlib.util
    spec = importlib.util.spec_from_file_location('pointnet_cli', os.path.join(REPO, 'pointnet.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    a = cli.parse([])
    assert (a.area, a.h5, a.ckpt, a.save, a.room_names, a.max_rooms, a.batch_rooms, a.device, a.metrics) == \
        ('1,2,3,4,5,6,scannet', None, None, None, None, 0, 68, None, 'host')
    assert cli.model_path(a, '3') == 'models/pointnet_model3.ckpt' and cli.model_path(a, 'scannet') == 'models/pointnet_model5.ckpt'
    a = cli.parse(['--h5', 'x.h5', '--area', 'kitti_val', '--ckpt', 'm.ckpt', '--save', '--metrics', 'device'])
    assert (a.area, a.h5, a.ckpt, a.save, a.metrics) == ('kitti_val', 'x.h5', 'm.ckpt', '', 'device')
    assert cli.model_path(a, 'kitti_val') == 'm.ckpt' and cli.MODE == 'pointnet'
    with pytest.raises(SystemExit):
        cli.parse(['--metrics', 'nowhere'])
