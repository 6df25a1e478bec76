"""CPU: the float64 restatement of the PointNet training step (tests/pointnet_train_ref.py) against finite differences and its own
edge cases, the host staging and jitter against their line-by-line twins, the checkpoint's tensors, the schedule, the C-ABI and the
command line's refusal of --mode pointnet2.  No GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointnet_ref                    # noqa: E402
import pointnet_train_ref as ref       # noqa: E402

TINY = ((32, 32), (32,), 3)
FD_STEP = 1e-6
FD_SEED = 0
FD_MARGIN = 2e-5                        # a step of 1e-6 on one weight moves a pre-activation by at most 1e-6 * |input| < 1e-5


def tiny_batch(seed, cells=3, rows=8, num_class=3):
    rs = np.random.RandomState(seed)
    pts = rs.uniform(-1, 1, (cells, rows, 6)).astype(np.float32)
    lab = rs.randint(0, num_class, (cells, rows))
    return pts, lab


def pre_activations(fw, w):
    """Every value a ReLU reads: the convolutions' and the batch norms' pre-activations."""
    out = []
    x = fw['points']
    for i, c in enumerate(fw['conv']):
        k = w['kernel%d' % i]
        out.append(x @ k.reshape(-1, k.shape[-1]).astype(np.float64) + w['bias%d' % i].astype(np.float64))
        x = c
    for j, z in enumerate(fw['zs']):
        beta, gamma = (w[n].astype(np.float64) for n in ref.bn_names(j)[:2])
        inv = gamma / np.sqrt(fw['variances'][j] + ref.BN_EPSILON)
        out.append(z * inv + (beta - fw['means'][j] * inv))
    return out


def test_gradients_agree_with_central_differences():
    conv, fc, ncls = TINY
    w = {k: v.astype(np.float64) for k, v in ref.init_like(FD_SEED, conv, fc, ncls, rows=8).items()}
    pts, lab = tiny_batch(FD_SEED + 100)
    fw, g = ref.loss_and_grads(pts, lab, w)
    # the test's own input: no ReLU input and no pool tie within reach of the difference step
    closest = min(float(np.abs(p).min()) for p in pre_activations(fw, w))
    assert closest > FD_MARGIN, 'a pre-activation at %g: choose another seed' % closest
    top = np.sort(fw['conv'][-1], axis=1)
    gap = (top[:, -1] - top[:, -2])[top[:, -1] > 0]
    assert gap.size and gap.min() > FD_MARGIN, 'a pool tie within %g: choose another seed' % gap.min()
    for name in ref.trainable_names(conv, fc):
        fd = np.zeros_like(w[name])
        flat, fdf = w[name].reshape(-1), fd.reshape(-1)
        for i in range(flat.size):
            keep = flat[i]
            flat[i] = keep + FD_STEP
            up = ref.forward(pts, lab, w)['loss']
            flat[i] = keep - FD_STEP
            dn = ref.forward(pts, lab, w)['loss']
            flat[i] = keep
            fdf[i] = (up - dn) / (2 * FD_STEP)
        scale = float(np.abs(g[name]).max())
        if name.startswith('fc_bias') and name != 'fc_bias%d' % len(fc):
            scale = float(np.abs(g[ref.bn_names(int(name[len('fc_bias'):]))[0]]).max())          # zero in exact arithmetic: beta's scale
        err = float(np.abs(fd - g[name]).max())
        assert err <= 1e-6 * scale, '%s: finite differences off by %g (largest entry %g)' % (name, err, scale)


def test_a_tied_pool_sends_its_gradient_to_the_first_row_and_the_weights_do_not_care():
    conv, fc, ncls = TINY
    w = {k: v.astype(np.float64) for k, v in ref.init_like(3, conv, fc, ncls, rows=8).items()}
    pts, lab = tiny_batch(5)
    pts[0, 6] = pts[0, 2]                                     # a cell drawn with replacement: rows 2 and 6 are one point
    lab[0, 6] = lab[0, 2]
    fw, first = ref.loss_and_grads(pts, lab, w, tie='first')
    _, last = ref.loss_and_grads(pts, lab, w, tie='last')
    last_conv, pooled = fw['conv'][-1], fw['pooled']
    tied = np.nonzero((last_conv[0, 2] == pooled[0]) & (pooled[0] > 0))[0]
    assert tied.size, 'the duplicated row wins no channel: choose another seed'
    assert np.all(first['_']['winner'][0, tied] == 2) and np.all(last['_']['winner'][0, tied] == 6)
    assert not np.array_equal(first['_']['dlast'], last['_']['dlast'])
    # column sums of the gradient of conv_last are zero either way (t = last - max(last) is shift invariant per cell and channel)
    for k in ref.trainable_names(conv, fc):
        scale = max(float(np.abs(first[k]).max()), 1e-30)
        assert float(np.abs(first[k] - last[k]).max()) <= 1e-12 * scale, k


def test_a_batch_of_one_cell_has_zero_variance_and_zero_gradient_through_the_batch_norm():
    conv, fc, ncls = TINY
    for dtype in (np.float64, np.float32):
        w = ref.init_like(1, conv, fc, ncls, rows=8)
        pts, lab = tiny_batch(2, cells=1)
        fw, g = ref.loss_and_grads(pts, lab, w, dtype)
        assert all(np.all(v == 0) for v in fw['variances'])
        assert all(np.all(dz == 0) for dz in g['_']['dz'])
        assert np.all(g['kernel0'] == 0) and np.abs(g['fc_weights%d' % len(fc)]).max() > 0


def test_hidden_fc_bias_gradients_vanish():
    for conv, fc, ncls in (TINY, ((32, 32, 64), (64, 32), 5)):
        w = ref.init_like(2, conv, fc, ncls, rows=8)
        pts, lab = tiny_batch(3, cells=4, num_class=ncls)
        _, g = ref.loss_and_grads(pts, lab, w)
        for j in range(len(fc)):
            beta = float(np.abs(g[ref.bn_names(j)[0]]).max())
            assert beta > 0
            assert float(np.abs(g['fc_bias%d' % j]).max()) < 1e-12 * beta


def room(seed, area):
    """A room with one cell over 2048 points, one under, and a few small ones; float32 rows x y z r g b."""
    rs = np.random.RandomState(seed)
    res = 3.0 if 'kitti' in area else 1.0
    big = rs.uniform(-0.49, 0.49, (2500, 2)) * res
    small = rs.uniform(-0.49, 0.49, (700, 2)) * res + np.array([res, 0.0])
    rest = rs.uniform(-2.4, 2.4, (300, 2)) * res
    xy = np.concatenate([big, small, rest])
    pts = np.concatenate([xy, rs.uniform(0.3, 2.5, (len(xy), 1)), rs.uniform(0, 1, (len(xy), 3))], axis=1).astype(np.float32)
    return pts, rs.randint(0, 13, len(xy))


@pytest.mark.parametrize('area', ['3', 'kitti_train'])
def test_stage_cells_and_jitter_equal_their_twins_bit_for_bit(area):
    from learn_region_grow_amd import pointnet_train as pt
    pts, cls = room(7, area)
    keep = pts.copy()
    got_p, got_l = pt.stage_cells(pts, cls, area, np.random.RandomState(11))
    want_p, want_l = ref.stage_cells(pts, cls, area, np.random.RandomState(11))
    assert np.array_equal(pts, keep), 'the room itself must not change'
    assert got_p.dtype == want_p.dtype == np.float32 and got_p.shape == want_p.shape and got_p.shape[1:] == (2048, 6)
    assert got_p.tobytes() == want_p.tobytes() and np.array_equal(got_l, want_l)
    sizes = sorted(len(np.unique(c, axis=0)) for c in got_p)
    assert sizes[-1] > 2048 * 0.6 and sizes[0] < 2048             # a cell drawn without and cells drawn with replacement
    assert len(got_p) >= 3
    if 'kitti' in area:
        assert np.abs(got_p[:, :, :2]).max() > 1.0                # cells of 3 m
    else:
        assert np.abs(got_p[:, :, :2]).max() <= 0.5 + 1e-6
    batch = got_p[:3, :1024].astype(np.float64)                   # the script jitters a float64 batch (:384, :403)
    a, b = pt.jitter(batch, np.random.RandomState(5)), ref.jitter(batch, np.random.RandomState(5))
    assert a.dtype == np.float64 and a.tobytes() == b.tobytes() and not np.array_equal(a, batch)


@pytest.mark.parametrize('arch', [pointnet_ref.SHIPPED, pointnet_ref.CURRENT])
def test_checkpoint_round_trip(arch, tmp_path):
    from learn_region_grow_amd import checkpoint
    conv, fc = arch
    w = pointnet_ref.random_weights(4, conv, fc, 13)
    rs = np.random.RandomState(0)
    names = ref.trainable_names(conv, fc)
    m = {k: rs.randn(*w[k].shape).astype(np.float32) for k in names}
    v = {k: rs.rand(*w[k].shape).astype(np.float32) for k in names}
    tensors = checkpoint.pointnet_checkpoint_tensors(w, m, v, step=7)
    prefix = str(tmp_path / 'pointnet_model5.ckpt')
    checkpoint.write_bundle(prefix, tensors)
    back = checkpoint.load_pointnet_weights(prefix)
    assert sorted(back) == sorted(w)
    for k in w:
        assert back[k].dtype == np.float32 and np.array_equal(back[k], w[k]), k
    everything = checkpoint.load_bundle(prefix)
    assert everything['Variable'].dtype == np.int32 and int(everything['Variable']) == 7
    assert everything['beta1_power'] == np.float32(0.9 ** 8) and everything['beta2_power'] == np.float32(0.999 ** 8)
    for k in names:
        assert np.array_equal(everything[k + '/Adam'], m[k]) and np.array_equal(everything[k + '/Adam_1'], v[k])
    for j in range(len(fc)):
        for n in checkpoint.pointnet_bn_names(j)[2:]:
            assert n in everything and n + '/Adam' not in everything and everything[n].shape == (1024, fc[j])
    if len(fc) > 1:
        assert checkpoint.pointnet_bn_names(1)[2].startswith('bn/bn_1/')
    assert len(everything) == 3 * len(names) + 2 * len(fc) + 3


def test_learning_rate_schedule():
    from learn_region_grow_amd import pointnet_train as pt
    for fn in (pt.learning_rate, ref.learning_rate):
        assert [fn(s) for s in (0, 499, 500, 1000)] == [2e-4, 2e-4, 1e-4, 5e-5]


def test_new_symbols_are_exported_and_the_abi_numbers_agree(hip_lib):
    from learn_region_grow_amd import _lib
    header = open(os.path.join(REPO, 'include', 'lrg_hip.h')).read()
    assert int(re.search(r'#define\s+LRG_ABI_VERSION\s+(\d+)', header).group(1)) == _lib.LRG_ABI_VERSION == hip_lib.lrg_abi_version() >= 16
    for name in ('lrg_pointnet_bn_forward', 'lrg_pointnet_bn_backward', 'lrg_pointnet_bn_backward_workspace_bytes',
                 'lrg_pointnet_softmax_ce_grad', 'lrg_pointnet_head_input', 'lrg_pointnet_head_input_backward', 'lrg_pointnet_ema_update'):
        assert hasattr(hip_lib, name) and name in _lib.EXPORTS and re.search(r'\b%s\s*\(' % name, header), name
    assert 'lrg_pointnet_train.hip' in _lib.SOURCES
    assert hasattr(hip_lib, 'lrg_gemm_f32_planes') and hip_lib.lrg_gemm_f32_planes_count(102400, 16) == 16 and hip_lib.lrg_gemm_f32_planes_count(0, 4) == 0
    assert hip_lib.lrg_pointnet_bn_backward_workspace_bytes(512) == 2 * 1024 * 512 * 4
    assert hip_lib.lrg_pointnet_bn_backward_workspace_bytes(48) == 0 and hip_lib.lrg_pointnet_bn_backward_workspace_bytes(544) == 0


def test_the_command_line_refuses_pointnet2_and_says_why():
    r = subprocess.run([sys.executable, os.path.join(REPO, 'train_pointnet.py'), '--mode', 'pointnet2'], capture_output=True, text=True)
    assert r.returncode != 0
    assert 'pointnet2' in r.stderr and 'DESIGN.md §7' in r.stderr
