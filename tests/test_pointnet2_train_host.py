"""CPU: the restatement of PointNet2's training step (tests/pointnet2_train_ref.py) against finite differences and under ties, the
checkpoint's key set, the new exports and the command line of train_pointnet2.py.  No GPU."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointnet2_ref                   # noqa: E402
import pointnet2_train_ref as ref      # noqa: E402

f32 = np.float32
SMALL_LEVELS = ((48, 0.35), (16, 0.6), (8, 1.0), (4, 2.0))       # cells of 48 rows; the network has 1024 and 1024 / 256 / 64 / 16
SMALL_SA = ((6, 5, 8), (7, 6, 9), (8, 7, 10), (9, 8, 12))
SMALL_FP = ((11, 10), (9, 8), (8, 7), (6, 6, 5))
NEW_SYMBOLS = ('lrg_pointnet2_group_mlp_train', 'lrg_pointnet2_row_mlp_train', 'lrg_pointnet2_scatter_grad')


def small_weights(seed, rgb, num_class=4):
    """The 46 trainables under their names at narrow widths, biases off zero so that ReLUs cut."""
    rs = np.random.RandomState(seed)
    feat = [3 if rgb else 0] + [m[-1] for m in SMALL_SA]
    shapes = {}
    for lv, mlp in enumerate(SMALL_SA):
        cin = 3 + feat[lv]
        for i, c in enumerate(mlp):
            shapes['layer%d/kernel%d' % (lv + 1, i)], shapes['layer%d/bias%d' % (lv + 1, i)] = (1, 1, cin, c), (c,)
            cin = c
    up = feat[4]
    for lv, mlp in enumerate(SMALL_FP):
        cin = up + feat[3 - lv]
        for i, c in enumerate(mlp):
            shapes['fa_layer%d/kernel%d' % (lv + 1, i)], shapes['fa_layer%d/bias%d' % (lv + 1, i)] = (1, 1, cin, c), (c,)
            cin = c
        up = mlp[-1]
    shapes.update({'kernel1': (1, up, 6), 'bias1': (6,), 'kernel2': (1, 6, num_class), 'bias2': (num_class,)})
    out = {}
    for k, shp in shapes.items():
        if 'kernel' in k:
            lim = np.sqrt(6.0 / (shp[-2] + shp[-1]))
            out[k] = rs.uniform(-lim, lim, shp)
        else:
            out[k] = rs.uniform(-0.1, 0.1, shp)
    return out


def small_batch(seed, n=48, distinct=(48, 20)):
    """Two cells: one of n distinct points, one of `distinct[1]` points drawn with replacement (ball-query padding and pool ties)."""
    rs = np.random.RandomState(seed)
    cells = []
    for d in distinct:
        p = rs.uniform(-0.5, 0.5, (d, 6)).astype(f32)
        p[:, 2] = rs.uniform(0, 1.5, d)
        pick = np.arange(n) if d == n else np.concatenate([np.arange(d), rs.randint(0, d, n - d)])
        cells.append(p[pick])
    pts = np.stack(cells)
    return pts, rs.randint(0, 4, (2, n))


def test_the_restatements_forward_is_pointnet2_refs():
    """On its own indices the training restatement's logits, level features and indices are tests/pointnet2_ref.forward's."""
    rs = np.random.RandomState(5)
    pts = rs.uniform(-0.5, 0.5, (1, 1024, 6)).astype(f32)
    pts[:, 600:] = pts[:, :424]
    w = pointnet2_ref.random_weights(3, 13, rgb_features=True)
    want, levels = pointnet2_ref.forward(pts, w, np.float64)
    ind = ref.level_indices(pts)
    fw = ref.forward(pts, np.zeros((1, 1024), int), w, ind, np.float64)
    for lv in range(4):
        assert np.array_equal(ind['sa'][lv]['fps'], levels['sa'][lv]['fps']) and np.array_equal(ind['sa'][lv]['idx'], levels['sa'][lv]['idx'])
        assert np.array_equal(ind['fp'][lv]['nn_idx'], levels['fp'][lv]['nn_idx'])
        assert np.array_equal(fw['feat'][lv + 1], levels['sa'][lv]['features'])
    assert np.array_equal(fw['logits'], want)


@pytest.mark.parametrize('rgb', [True, False])
def test_gradients_against_finite_differences(rgb):
    """Central differences of the float64 loss with the indices frozen, four entries of each of the 46 tensors.  An entry whose
    one-sided differences disagree sits at a ReLU or pool kink and is skipped; at most 5 % of the probes may be."""
    pts, lab = small_batch(11)
    w = small_weights(7, rgb)
    ind = ref.level_indices(pts, SMALL_LEVELS)
    fw, g = ref.loss_and_grads(pts, lab, w, ind)
    assert len(w) == 46 and sorted(g) == sorted(w)
    f0, h = fw['loss'], 1e-6
    rs = np.random.RandomState(1)
    probes = skipped = 0
    worst = 0.0
    for k in sorted(w):
        scale = max(float(np.abs(g[k]).max()), 1e-3)
        assert g[k].shape == w[k].shape and np.abs(g[k]).max() > 0, k
        for flat in rs.choice(w[k].size, min(4, w[k].size), replace=False):
            at = np.unravel_index(flat, w[k].shape)
            vals = []
            for sign in (1, -1):
                w2 = dict(w)
                w2[k] = w[k].copy()
                w2[k][at] += sign * h
                vals.append(ref.forward(pts, lab, w2, ind)['loss'])
            fwd, bwd, mid = (vals[0] - f0) / h, (f0 - vals[1]) / h, (vals[0] - vals[1]) / (2 * h)
            probes += 1
            if abs(fwd - bwd) > 1e-3 * scale:
                skipped += 1
                continue
            err = abs(mid - g[k][at]) / scale
            worst = max(worst, err)
            assert err <= 1e-5, (k, at, mid, g[k][at])
    print('probes %d skipped %d worst relative error %.2e' % (probes, skipped, worst))
    assert probes >= 46 * 3 and skipped <= 0.05 * probes


def test_weight_gradients_do_not_depend_on_which_duplicate_is_listed():
    """A cell whose rows are duplicates of five points: naming, in every ball query and every three_nn list, another copy of the same
    point leaves the loss and every weight gradient where it was."""
    rs = np.random.RandomState(2)
    base = rs.uniform(-0.3, 0.3, (5, 6)).astype(f32)
    which = np.concatenate([np.arange(5), rs.randint(0, 5, 43)])
    pts = base[which][None]
    lab = (which % 4)[None]
    w = small_weights(9, True)
    ind = ref.level_indices(pts, SMALL_LEVELS)
    fw, g = ref.loss_and_grads(pts, lab, w, ind)
    # the points of every level, to find each one's copies
    xyz = [pts[:, :, :3]]
    for lv in range(4):
        xyz.append(xyz[-1][np.arange(1)[:, None], ind['sa'][lv]['fps']])

    def last_copy(level_xyz, idx):
        same = (level_xyz[0][:, None, :] == level_xyz[0][None, :, :]).all(axis=2)           # [n, n]
        last = same.shape[0] - 1 - same[:, ::-1].argmax(axis=1)
        return last[idx].astype(np.int32)
    other = dict(sa=[dict(fps=ind['sa'][lv]['fps'], idx=last_copy(xyz[lv], ind['sa'][lv]['idx'])) for lv in range(4)],
                 fp=[dict(nn_idx=last_copy(xyz[4 - lv], ind['fp'][lv]['nn_idx']), weight=ind['fp'][lv]['weight']) for lv in range(4)])
    assert any((other['sa'][lv]['idx'] != ind['sa'][lv]['idx']).any() for lv in range(4))
    fw2, g2 = ref.loss_and_grads(pts, lab, w, other)
    assert abs(fw2['loss'] - fw['loss']) <= 1e-13
    for k in sorted(g):
        np.testing.assert_allclose(g2[k], g[k], rtol=0, atol=1e-12 * max(1.0, np.abs(g[k]).max()), err_msg=k)


def test_checkpoint_tensors_have_the_shipped_key_set(tmp_path):
    from learn_region_grow_amd import checkpoint
    from learn_region_grow_amd.pointnet2_train import initial_weights
    golden = json.load(open(os.path.join(GOLDEN, 'pointnet2_model5_names.json')))
    w = initial_weights(13, rgb_features=False, seed=1)
    m = {k: np.full(v.shape, 0.5, f32) for k, v in w.items()}
    t = checkpoint.pointnet2_checkpoint_tensors(w, m, None, step=7)
    assert sorted(t) == sorted(golden)
    for k, shp in golden.items():
        assert list(np.shape(t[k])) == list(shp), k
    assert t['Variable'] == 7 and t['Variable'].dtype == np.int32
    assert t['beta1_power'] == f32(0.9 ** 8) and t['beta2_power'] == f32(0.999 ** 8)
    assert (t['kernel1/Adam'] == 0.5).all() and not t['kernel1/Adam_1'].any()
    # kernels in the initialiser's range, biases zero
    assert not w['layer3/bias1'].any() and 0 < np.abs(w['layer1/kernel0']).max() <= np.sqrt(6.0 / (3 + 32))
    for rgb, ncls in ((False, 13), (True, 13), (True, 260)):
        w = initial_weights(ncls, rgb_features=rgb, seed=2)
        prefix = str(tmp_path / ('m_%d_%d.ckpt' % (rgb, ncls)))
        checkpoint.write_bundle(prefix, checkpoint.pointnet2_checkpoint_tensors(w, step=3))
        back = checkpoint.load_pointnet2_weights(prefix)
        assert checkpoint.pointnet2_variant({k: v.shape for k, v in back.items()}) == (ncls, rgb)
        assert sorted(back) == sorted(w) and all(np.array_equal(back[k], w[k]) for k in w)
    with pytest.raises(KeyError):
        checkpoint.pointnet2_checkpoint_tensors({k: v for k, v in w.items() if k != 'fa_layer2/bias1'})


def test_new_entry_points_are_declared_bound_and_exported(hip_lib):
    from learn_region_grow_amd import _lib
    header = open(os.path.join(REPO, 'include', 'lrg_hip.h')).read()
    for name in NEW_SYMBOLS:
        assert re.search(r'^int %s\(' % name, header, flags=re.M), name
        assert name in _lib.EXPORTS and hasattr(hip_lib, name), name
    assert 'lrg_pointnet2_train.hip' in _lib.SOURCES


def test_command_line_help_and_output_names():
    r = subprocess.run([sys.executable, os.path.join(REPO, 'train_pointnet2.py'), '--help'], capture_output=True, text=True)
    assert r.returncode == 0 and '--features' in r.stdout and '[--features {rgb,xyz}]' in r.stdout and '[--arch' not in r.stdout
    sys.path.insert(0, REPO)
    import train_pointnet
    import train_pointnet2
    a = train_pointnet2.parse([])
    assert (a.mode, a.features, a.batch_size) == ('pointnet2', 'rgb', 100)
    assert train_pointnet.model_path(a) == os.path.join('models', 'pointnet2_model5.ckpt')
    a = train_pointnet2.parse(['--cross-domain', '--train-area', 'kitti_train', '--val-area', 'kitti_val'])
    assert train_pointnet.model_path(a) == os.path.join('models', 'cross_domain', 'pointnet2_kitti_train.ckpt')
    assert train_pointnet.num_classes(a.train_area) == 260
