"""GPU: the training side of PointNet2 (csrc/lrg_pointnet2_train.hip, the KEEP form of csrc/lrg_pointnet2.hip,
learn_region_grow_amd/pointnet2_train.py, train_pointnet2.py) against the float64 restatement tests/pointnet2_train_ref.py.

The bound is the project's own (tests/test_gpu_pointnet_train.py::within): an error against float64 is at most
max(8 * err32, 2e-5 * scale), err32 the float32 restatement's own error on the same inputs and scale the tensor's largest magnitude;
losses rtol 2e-5.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointnet2_ref as R              # noqa: E402
import pointnet2_train_ref as ref      # noqa: E402
from trainer_helpers import adam_f32, bits, three_cells      # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
EINVAL = -1000
P = 1024
I32P = ctypes.POINTER(ctypes.c_int32)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def dev(a, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def within(name, got, want64, want32, scale=None):
    scale = float(np.abs(want64).max()) if scale is None else scale
    err32 = float(np.abs(np.asarray(want32, np.float64) - want64).max())
    err = float(np.abs(np.asarray(got, np.float64) - want64).max())
    tol = max(8 * err32, 2e-5 * scale)
    print('%-44s scale %.3e  gpu err %.3e  f32 err %.3e  gpu/tol %.3f' % (name, scale, err, err32, err / max(tol, 1e-300)))
    assert np.isfinite(np.asarray(got)).all(), name
    assert err <= tol, name


def pack(lib, layers, device):
    import torch
    sizes = [lib.lrg_pointnet2_packed_floats(w.shape[0], w.shape[1]) for w, _ in layers]
    packed = torch.zeros(sum(sizes), dtype=torch.float32, device=device)
    off = 0
    for (w, b), s in zip(layers, sizes):
        wd, bd = dev(w, device), dev(b, device)
        assert lib.lrg_pointnet2_pack_layer(w.shape[0], w.shape[1], ptr(wd), ptr(bd), ptr(packed[off:]), None) == 0
        off += s
    torch.cuda.synchronize()
    return packed


# ---------------------------------------------------------------- the ordered scatter ----------------------------------------------------------------
def scatter_np(n, per, c, grad, col0, idx, weight, drop, addend, mask, dtype):
    """np.add.at in ascending entry order, per batch element."""
    b, q = grad.shape[:2]
    out = np.zeros((b, n, c), dtype) if addend is None else addend.astype(dtype).copy()
    acc = np.zeros((b, n, c), dtype)
    for bi in range(b):
        j = idx[bi].astype(np.int64)
        ok = (j >= 0) & (j < n)
        e = np.arange(q * per)
        vals = grad[bi, e // per, col0:col0 + c].astype(dtype)
        if weight is not None:
            vals = vals * weight[bi][:, None].astype(dtype)
        if drop:
            np.add.at(acc[bi], j[ok], vals[ok])
        else:
            np.add.at(acc[bi], np.where(ok, j, 0), vals)
    out = out + acc
    if mask is not None:
        out = np.where(mask > 0, out, dtype(0))
    return out


def run_scatter(lib, device, n, per, c, grad, col0, idx, weight, drop, addend, mask, in_place=False):
    import torch
    b, q, ldg = grad.shape
    t = [dev(grad, device), dev(idx.astype(np.int32), device), None if weight is None else dev(weight, device),
         None if addend is None else dev(addend, device), None if mask is None else dev(mask, device)]
    out = t[3] if in_place else torch.full((b, n, c), float('nan'), dtype=torch.float32, device=device)
    rc = lib.lrg_pointnet2_scatter_grad(b, n, q, per, c, ptr(t[0]), ldg, col0, ptr(t[1]), ptr(t[2]), drop, ptr(t[3]), ptr(t[4]), ptr(out), None)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


SCATTER_CASES = {'group': dict(b=2, n=7, q=3 * 32, per=1, c=5, ldg=8, col0=3, weighted=False, drop=0),
                 'interpolate': dict(b=2, n=4, q=9, per=3, c=33, ldg=33, col0=0, weighted=True, drop=1),
                 'two-slabs': dict(b=2, n=300, q=40 * 32, per=1, c=3, ldg=6, col0=3, weighted=False, drop=0)}


@pytest.mark.parametrize('name', sorted(SCATTER_CASES))
def test_scatter_grad_adds_in_ascending_entry_order(hip_lib, cuda_device, name):
    """Heavy repeats, one source nobody names, one index out of range of each kind (below 0, at n); against np.add.at in float64 under
    the bound; the float32 np.add.at (ascending entries) bit for bit; two runs and the cells in the opposite batch order give the
    same bits per cell; the addend (in place too) and the mask."""
    k = SCATTER_CASES[name]
    b, n, q, per, c = k['b'], k['n'], k['q'], k['per'], k['c']
    rs = np.random.RandomState(len(name))
    grad = rs.randn(b, q, k['ldg']).astype(f32)
    idx = rs.randint(0, n - 1, (b, q * per)).astype(np.int32)          # source n - 1 is never named
    idx[:, : q * per // 2] = idx[:, :1]                                # half of the entries name one source
    idx[0, 3], idx[1, 5] = -1, n                                       # out of range, both kinds
    weight = rs.uniform(0.1, 1, (b, q * per)).astype(f32) if k['weighted'] else None
    args = (n, per, c, grad, k['col0'], idx, weight, k['drop'])
    rc, got = run_scatter(hip_lib, cuda_device, *args, None, None)
    assert rc == 0
    w64, w32 = scatter_np(*args, None, None, np.float64), scatter_np(*args, None, None, np.float32)
    within(name, got, w64, w32)
    assert np.array_equal(bits(got), bits(w32)), 'the sum must run in ascending entry order'
    assert not bits(got[:, n - 1]).any(), 'a row nobody names is written as zero'
    moved = scatter_np(n, per, c, grad, k['col0'], np.where((idx < 0) | (idx >= n), 1, idx), weight, k['drop'], None, None, np.float64)
    assert np.abs(moved - w64).max() > 0                               # where the out-of-range entries go matters on these inputs
    assert np.array_equal(bits(run_scatter(hip_lib, cuda_device, *args, None, None)[1]), bits(got))
    flip = lambda a: None if a is None else a[::-1]
    rc, rev = run_scatter(hip_lib, cuda_device, n, per, c, flip(grad), k['col0'], flip(idx), flip(weight), k['drop'], None, None)
    assert rc == 0 and np.array_equal(bits(rev[::-1]), bits(got))
    addend = rs.randn(b, n, c).astype(f32)
    mask = rs.randn(b, n, c).astype(f32)
    mask[0, 0, 0] = 0                                                  # zero counts as cut
    want = np.where(mask > 0, addend + w32, f32(0))
    for in_place in (False, True):
        rc, full = run_scatter(hip_lib, cuda_device, *args, addend, mask, in_place)
        assert rc == 0 and np.array_equal(bits(full), bits(want)), in_place
    rc, only = run_scatter(hip_lib, cuda_device, *args, addend, None)
    assert np.array_equal(bits(only[:, n - 1]), bits(addend[:, n - 1])), 'a row nobody names gets the addend alone'


# ---------------------------------------------------------------- the forward that keeps its layers ----------------------------------------------------------------
@pytest.mark.parametrize('c,widths', [(0, (32, 32, 64)), (3, (32, 32, 64)), (64, (64, 64, 128))])
def test_group_mlp_train_keeps_its_layers(hip_lib, cuda_device, c, widths):
    import torch
    rng = np.random.RandomState(c + widths[0])
    layers = R.random_layers(rng, (3 + c,) + widths)
    packed = pack(hip_lib, layers, cuda_device)
    b, n, m = 2, 40, 5
    xyz = rng.uniform(0, 1, (b, n, 3)).astype(f32)
    new_xyz = rng.uniform(0, 1, (b, m, 3)).astype(f32)
    points = rng.uniform(-1, 1, (b, n, c)).astype(f32) if c else None
    idx = rng.randint(0, n, (b, m, 32)).astype(np.int32)
    idx[:, 0, 5:] = idx[:, 0, :1]                                      # the ball query's padding
    idx[0, 1, 2], idx[1, 2, 3] = -1, n                                 # out of range: row 0
    t = [dev(xyz, cuda_device), dev(new_xyz, cuda_device), None if c == 0 else dev(points, cuda_device), dev(idx, cuda_device)]
    wd = np.array(widths, np.int32)
    nan = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=cuda_device)
    plain, out, rows = nan(b, m, widths[2]), nan(b, m, widths[2]), nan(b * m * 32, 3 + c)
    keep = [nan(b * m * 32, w) for w in widths]
    assert hip_lib.lrg_pointnet2_group_mlp(b, n, m, 32, c, ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(t[3]), wd.ctypes.data_as(I32P), ptr(packed), ptr(plain),
                                           None) == 0
    assert hip_lib.lrg_pointnet2_group_mlp_train(b, n, m, 32, c, ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(t[3]), wd.ctypes.data_as(I32P), ptr(packed),
                                                 ptr(out), ptr(rows), ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(plain.cpu().numpy()))
    use = np.where((idx < 0) | (idx >= n), 0, idx)
    bi = np.arange(b)[:, None, None]
    g = xyz[bi, use] - new_xyz[:, :, None, :]
    want_rows = g if c == 0 else np.concatenate([g, points[bi, use]], axis=-1)
    assert np.array_equal(bits(rows.cpu().numpy()), bits(want_rows.reshape(-1, 3 + c)))
    for L in range(3):
        w64 = R.row_mlp(want_rows.reshape(-1, 3 + c), None, layers[:L + 1], True, np.float64)
        w32 = R.row_mlp(want_rows.reshape(-1, 3 + c), None, layers[:L + 1], True, np.float32)
        within('group keep%d c %d widths %s' % (L, c, widths), keep[L].cpu().numpy(), w64, w32)
    # the pooled output is the maximum of the kept last layer, bit for bit
    assert np.array_equal(bits(keep[2].cpu().numpy().reshape(b, m, 32, -1).max(axis=2)), bits(out.cpu().numpy()))
    # every extra output is optional
    again = nan(b, m, widths[2])
    assert hip_lib.lrg_pointnet2_group_mlp_train(b, n, m, 32, c, ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(t[3]), wd.ctypes.data_as(I32P), ptr(packed),
                                                 ptr(again), None, None, None, None, None) == 0
    assert np.array_equal(bits(again.cpu().numpy()), bits(plain.cpu().numpy()))


@pytest.mark.parametrize('r', [1, 33])
@pytest.mark.parametrize('ca,cb,widths,relu_last', [(128, 3, (128, 128, 128), 1), (128, 0, (128, 13), 0), (20, 5, (13,), 0)])
def test_row_mlp_train_keeps_its_layers(hip_lib, cuda_device, ca, cb, widths, relu_last, r):
    import torch
    rng = np.random.RandomState(ca + cb + len(widths) + r)
    layers = R.random_layers(rng, (ca + cb,) + widths)
    packed = pack(hip_lib, layers, cuda_device)
    a, b2 = rng.uniform(-1, 1, (r, ca)).astype(f32), rng.uniform(-1, 1, (r, cb)).astype(f32) if cb else None
    ta, tb = dev(a, cuda_device), None if cb == 0 else dev(b2, cuda_device)
    wd = np.array(widths, np.int32)
    nan = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=cuda_device)
    plain, out = nan(r, widths[-1]), nan(r, widths[-1])
    keep = [nan(r, w) for w in widths] + [None, None]
    assert hip_lib.lrg_pointnet2_row_mlp(r, ca, cb, ptr(ta), ptr(tb), len(widths), wd.ctypes.data_as(I32P), relu_last, ptr(packed), ptr(plain), None) == 0
    assert hip_lib.lrg_pointnet2_row_mlp_train(r, ca, cb, ptr(ta), ptr(tb), len(widths), wd.ctypes.data_as(I32P), relu_last, ptr(packed), ptr(out),
                                               ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(plain.cpu().numpy()))
    assert np.array_equal(bits(keep[len(widths) - 1].cpu().numpy()), bits(out.cpu().numpy())), 'the last kept layer repeats out'
    for L in range(len(widths)):
        last = L == len(widths) - 1
        w64 = R.row_mlp(a, b2, layers[:L + 1], bool(relu_last) or not last, np.float64)
        w32 = R.row_mlp(a, b2, layers[:L + 1], bool(relu_last) or not last, np.float32)
        within('row keep%d (%d, %d) widths %s r %d' % (L, ca, cb, widths, r), keep[L].cpu().numpy(), w64, w32)
    if not relu_last:
        assert (out.cpu().numpy() < 0).any()


def test_bad_arguments(hip_lib, cuda_device):
    """The error codes the header documents; nothing is launched (the outputs keep their zeros)."""
    import torch
    a = torch.zeros(1 << 16, dtype=torch.float32, device=cuda_device)
    i = torch.zeros(1 << 12, dtype=torch.int32, device=cuda_device)
    L, p, ip = hip_lib, ptr(a), ptr(i)
    ok = lambda **kw: dict(dict(b=1, n=4, q=8, per=1, c=2, grad=p, ldg=4, col0=2, idx=ip, weight=None, drop=0, addend=None, mask=None, out=p), **kw)
    call = lambda **kw: L.lrg_pointnet2_scatter_grad(*[ok(**kw)[k] for k in ('b', 'n', 'q', 'per', 'c', 'grad', 'ldg', 'col0', 'idx', 'weight', 'drop',
                                                                         'addend', 'mask', 'out')], None)
    assert call(b=0) == 0
    for bad in (dict(grad=None), dict(idx=None), dict(out=None)):
        assert call(**bad) == EINVAL - 1, bad
    for bad in (dict(b=-1), dict(b=65536), dict(n=0), dict(q=0), dict(per=0), dict(c=0), dict(col0=-1), dict(col0=3), dict(ldg=0), dict(q=16385),
                dict(q=8192, per=3), dict(drop=2)):
        assert call(**bad) == EINVAL - 2, bad
    # the _train forms check what the inference forms check: widths, nsample, 3 + c
    wd = lambda *w: np.array(w, np.int32).ctypes.data_as(I32P)
    group = lambda ns=32, c=3, w=(32, 32, 64), out=p: L.lrg_pointnet2_group_mlp_train(1, 40, 2, ns, c, p, p, p, ip, wd(*w), p, out, p, p, p, p, None)
    plain = lambda ns=32, c=3, w=(32, 32, 64), out=p: L.lrg_pointnet2_group_mlp(1, 40, 2, ns, c, p, p, p, ip, wd(*w), p, out, None)
    for kw in (dict(ns=16), dict(ns=33), dict(c=1022), dict(c=-1), dict(w=(33, 32, 64)), dict(w=(32, 32, 65)), dict(w=(544, 32, 64)), dict(out=None)):
        assert EINVAL - 100 < group(**kw) <= EINVAL and group(**kw) == plain(**kw), kw
    rows = lambda r=5, ca=6, cb=3, n=3, w=(64, 32, 13), relu=1, out=p: L.lrg_pointnet2_row_mlp_train(r, ca, cb, p, p, n, wd(*w), relu, p, out, p, p, p, None)
    rplain = lambda r=5, ca=6, cb=3, n=3, w=(64, 32, 13), relu=1, out=p: L.lrg_pointnet2_row_mlp(r, ca, cb, p, p, n, wd(*w), relu, p, out, None)
    for kw in (dict(r=-1), dict(ca=0), dict(ca=1000, cb=25), dict(n=0), dict(n=4), dict(w=(63, 32, 13)), dict(w=(64, 32, 513)), dict(relu=2), dict(out=None)):
        assert EINVAL - 100 < rows(**kw) <= EINVAL and rows(**kw) == rplain(**kw), kw
    assert rows(r=0) == 0
    torch.cuda.synchronize()
    assert not a.any()


# ---------------------------------------------------------------- the trainer ----------------------------------------------------------------
TRAINER_CASES = {'rgb-13': (13, True), 'xyz-13': (13, False), 'rgb-260': (260, True)}
_cases = {}


def trainer_case(name):
    """Weights, a batch, the restatement's own level indices and its answers on them (float64 and float32), computed once per case and
    left unchanged."""
    if name in _cases:
        return _cases[name]
    ncls, rgb = TRAINER_CASES[name]
    seed = sorted(TRAINER_CASES).index(name)
    w = R.random_weights(30 + seed, ncls, rgb)                        # biases off zero: every term of the gradient is exercised
    pts = three_cells(50 + seed)
    rs = np.random.RandomState(70 + seed)
    lab = rs.randint(0, ncls, (3, P))
    ind = ref.level_indices(pts)
    fw64, g64 = ref.loss_and_grads(pts, lab, w, ind, np.float64)
    fw32, g32 = ref.loss_and_grads(pts, lab, w, ind, np.float32)
    _cases[name] = dict(w=w, pts=pts, lab=lab, ind=ind, fw=fw64, fw32=fw32, G=g64, G32=g32, ncls=ncls, rgb=rgb, B=3)
    return _cases[name]


def make_trainer(case, device, **kw):
    from learn_region_grow_amd.pointnet2_train import PointNet2Trainer
    return PointNet2Trainer(case['B'], case['ncls'], case['rgb'], device=device, **kw).load_weights(case['w'])


def same_indices(got, want):
    for lv in range(4):
        assert np.array_equal(got['sa'][lv]['fps'], want['sa'][lv]['fps']), lv
        assert np.array_equal(got['sa'][lv]['idx'], want['sa'][lv]['idx']), lv
        assert np.array_equal(got['fp'][lv]['nn_idx'], want['fp'][lv]['nn_idx']), lv
        assert np.array_equal(bits(got['fp'][lv]['weight']), bits(want['fp'][lv]['weight'])), lv


@pytest.mark.parametrize('name', sorted(TRAINER_CASES))
def test_backward_matches_the_restatement(cuda_device, name):
    """The level indices first (xyz only: bit for bit the restatement's), then on them the loss (rtol 2e-5), the accuracy up to the
    rows whose two largest float64 logits are within the logits' bound, and all 46 gradients."""
    case = trainer_case(name)
    tr = make_trainer(case, cuda_device)
    tr.gflat.fill_(float('nan'))
    sc = tr.backward(case['pts'], case['lab'])
    same_indices(tr.level_indices(), case['ind'])
    fw, fw32 = case['fw'], case['fw32']
    print('loss %.6f (restatement %.6f)  acc %.4f (%.4f)' % (sc['loss'], fw['loss'], sc['acc'], fw['acc']))
    np.testing.assert_allclose(sc['loss'], fw['loss'], rtol=2e-5)
    logits = tr.train_logits().cpu().numpy()
    within('logits', logits, fw['logits'], fw32['logits'])
    tol = max(8 * np.abs(fw32['logits'] - fw['logits']).max(), 2e-5 * np.abs(fw['logits']).max())
    top = np.sort(fw['logits'], axis=2)
    close = int(((top[..., -1] - top[..., -2]) <= 2 * tol).sum())
    assert abs(sc['acc'] - fw['acc']) * case['B'] * P <= close + 1e-6
    got = tr.grads_numpy()
    assert sorted(got) == sorted(case['G']) and len(got) == 46
    for k in sorted(got):
        within(k, got[k], case['G'][k], case['G32'][k])
    # evaluate-style call: loss only, nothing else touched
    tr.gflat.fill_(-777.25)
    assert tr.backward(case['pts'], case['lab'], loss_only=True) == sc
    assert (tr.gflat == -777.25).all()


def test_train_step_is_adam_at_a_constant_rate_on_the_trainers_own_gradients(cuda_device):
    case = trainer_case('xyz-13')
    tr = make_trainer(case, cuda_device)
    flat = lambda d: np.concatenate([d[k].reshape(-1) for k in tr.names])
    p, m, v = flat(tr.weights_numpy()), np.zeros(tr.flat.numel(), f32), np.zeros(tr.flat.numel(), f32)
    for step in range(2):
        assert tr.step == step
        tr.train_step(case['pts'], case['lab'])
        g, t = flat(tr.grads_numpy()), step + 1
        p, m, v = adam_f32(p, g, m, v, 0.001 * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t), 0.9, 0.999, 1e-8)
        for what, got, want in (('weights', tr.flat, p), ('m', tr.m, m), ('v', tr.v, v)):
            bad = bits(got.cpu().numpy()) != bits(want)
            assert not bad.any(), 'step %d %s: %d of %d differ' % (step, what, bad.sum(), bad.size)
        sm, sv = tr.slots_numpy()
        assert np.array_equal(bits(flat(sm)), bits(m)) and np.array_equal(bits(flat(sv)), bits(v))
    assert tr.step == 2


def test_three_steps_twice_give_the_same_bits(cuda_device):
    case = trainer_case('rgb-13')
    runs = []
    for _ in range(2):
        tr = make_trainer(case, cuda_device)
        rs = np.random.RandomState(3)
        for step in range(3):
            tr.train_step(case['pts'] + rs.uniform(-0.01, 0.01, case['pts'].shape).astype(f32), case['lab'])
        runs.append([bits(t.cpu().numpy()) for t in (tr.flat, tr.m, tr.v, tr.gflat)])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


@pytest.mark.parametrize('name', ['rgb-13', 'xyz-13'])
def test_training_forward_evaluation_and_saved_checkpoint_agree(cuda_device, tmp_path, name):
    from learn_region_grow_amd import checkpoint
    from learn_region_grow_amd.pointnet2 import PointNet2HIP
    case = trainer_case(name)
    tr = make_trainer(case, cuda_device)
    tr.train_step(case['pts'], case['lab'])
    sc = tr.backward(case['pts'], case['lab'], loss_only=True)        # the training forward on the updated weights
    trained = tr.train_logits().cpu().numpy()
    behind = tr.eval_logits(case['pts']).cpu().numpy()
    assert np.array_equal(bits(trained), bits(behind))
    assert tr.evaluate(case['pts'], case['lab']) == sc
    prefix = str(tmp_path / 'models' / 'pointnet2_model5.ckpt')
    tr.save(prefix)
    back = checkpoint.load_pointnet2_weights(prefix)
    now = tr.weights_numpy()
    assert all(np.array_equal(bits(back[k]), bits(now[k])) for k in now)
    everything = checkpoint.load_bundle(prefix)
    assert int(everything['Variable']) == 1 and everything['kernel1/Adam'].any() and 'beta2_power' in everything
    assert np.array_equal(bits(PointNet2HIP(back, device=cuda_device).logits(case['pts'])), bits(behind))


def band_batch(B=4, ncls=3):
    """The class of a point is its height band: 0 .. 1 m, 1 .. 2 m, 2 .. 3 m."""
    rs = np.random.RandomState(0)
    p = rs.uniform(-0.5, 0.5, (B, P, 6)).astype(f32)
    p[:, :, 2] = rs.uniform(0, 3, (B, P))
    return p, np.minimum(p[:, :, 2].astype(int), ncls - 1)


def test_it_learns(cuda_device):
    """Twelve steps of Adam at 0.001 on four cells whose classes are height bands: the float64 restatement, run with the same updates
    on the same indices, loses more than a tenth of its starting loss (1.099 -> 0.881 on the CPU); the GPU trainer's loss must fall by
    at least half of that drop.  (A step of the restatement at B = 4 costs most of a second, which is what keeps this at a dozen.)"""
    from learn_region_grow_amd.pointnet2_train import PointNet2Trainer, initial_weights
    steps = 12
    pts, lab = band_batch()
    w = initial_weights(3, True, seed=0)
    tr = PointNet2Trainer(4, 3, True, device=cuda_device).load_weights(w)
    got = [tr.train_step(pts, lab)['loss'] for _ in range(steps)]
    ind = ref.level_indices(pts)
    same_indices(tr.level_indices(), ind)
    _, want = ref.train([(pts, lab, ind)] * steps, w)
    drop = want[0] - want[-1]
    print('restatement %.4f -> %.4f, trainer %.4f -> %.4f' % (want[0], want[-1], got[0], got[-1]))
    assert drop >= 0.1 * want[0]
    np.testing.assert_allclose(got[0], want[0], rtol=2e-5)
    assert got[0] - got[-1] >= 0.5 * drop


def test_labels_out_of_range_raise(cuda_device):
    case = trainer_case('xyz-13')
    tr = make_trainer(case, cuda_device)
    lab = case['lab'].copy()
    lab[1, 7] = 13
    with pytest.raises(ValueError):
        tr.backward(case['pts'], lab)
    lab[1, 7] = -1
    with pytest.raises(ValueError):
        tr.evaluate(case['pts'], lab)


def test_a_batch_of_one_cell(cuda_device):
    from learn_region_grow_amd.pointnet2_train import PointNet2Trainer
    case = trainer_case('rgb-13')
    three = make_trainer(case, cuda_device)
    three.backward(case['pts'], case['lab'], loss_only=True)
    one = PointNet2Trainer(1, 13, True, device=cuda_device).load_weights(case['w'])
    sc = one.train_step(case['pts'][1:2], case['lab'][1:2])
    assert np.isfinite(sc['loss']) and one.step == 1
    assert np.array_equal(bits(one.train_logits().cpu().numpy()[0]), bits(three.train_logits().cpu().numpy()[1])), 'a cell does not see its batch'
    assert all(np.isfinite(g).all() and g.any() for g in one.grads_numpy().values())


def test_command_line_trains_and_the_checkpoint_runs(cuda_device, tmp_path):
    from learn_region_grow_amd import checkpoint, io, synthetic
    raw = [synthetic.area5_shaped_room(2500, 11).astype(f32), synthetic.area5_shaped_room(1800, 12).astype(f32)]
    data = tmp_path / 'data'
    data.mkdir()
    h5 = str(data / 's3dis_area1.h5')
    io.saveToH5(h5, raw)
    p = subprocess.run([sys.executable, os.path.join(REPO, 'train_pointnet2.py'), '--train-area', '1', '--val-area', '1', '--data-dir', str(data),
                        '--model-dir', str(tmp_path / 'models'), '--epochs', '1', '--val-step', '1', '--batch-size', '2', '--features', 'xyz'],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.split('\n')
    assert any(l.startswith('Epoch: 0 Loss: ') and '(cls ' in l for l in lines), p.stdout[-2000:]
    assert any(l.startswith('Validation: 0 Loss: ') for l in lines), p.stdout[-2000:]
    ck = str(tmp_path / 'models' / 'pointnet2_model1.ckpt')
    w = checkpoint.load_pointnet2_weights(ck)
    assert checkpoint.pointnet2_variant({k: v.shape for k, v in w.items()}) == (13, False)
    assert int(checkpoint.load_bundle(ck, names=['Variable'])['Variable']) >= 1
    p = subprocess.run([sys.executable, os.path.join(REPO, 'pointnet2.py'), '--h5', h5, '--area', '1', '--ckpt', ck], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert 'Restored from %s' % ck in p.stdout
