"""GPU: the training side of the plain PointNet (csrc/lrg_pointnet_train.hip, learn_region_grow_amd/pointnet_train.py) against the
float64 restatement tests/pointnet_train_ref.py.

The bound is the project's own (tests/test_gpu_train_kernels.py): an error against float64 is at most
max(8 * err32, 2e-5 * scale), err32 the float32 restatement's own error and scale the tensor's largest magnitude; losses rtol 2e-5.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointnet_ref                    # noqa: E402
import pointnet_train_ref as ref       # noqa: E402
from trainer_helpers import adam_f32, bits      # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32
EINVAL = -1000
P = 1024


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev_of(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def within(name, got, want64, want32, scale=None):
    scale = float(np.abs(want64).max()) if scale is None else scale
    err32 = float(np.abs(np.asarray(want32, np.float64) - want64).max())
    err = float(np.abs(np.asarray(got, np.float64) - want64).max())
    tol = max(8 * err32, 2e-5 * scale)
    print('%-44s scale %.3e  gpu err %.3e  f32 err %.3e  gpu/tol %.3f' % (name, scale, err, err32, err / max(tol, 1e-300)))
    assert np.isfinite(np.asarray(got)).all(), name
    assert err <= tol, name


# ---------------------------------------------------------------- batch norm ----------------------------------------------------------------
def bn_backward_np(z, y, dy, mean, var, gamma, dtype):
    z, y, dy, mean, var, gamma = (a.astype(dtype) for a in (z, y, dy, mean, var, gamma))
    n = dtype(z.shape[0])
    g = np.where(y > 0, dy, dtype(0))
    rstd = dtype(1) / np.sqrt(var + dtype(1e-3))
    xhat = (z - mean) * rstd
    dz = gamma * rstd * (g - g.sum(axis=0) / n - xhat * ((g * xhat).sum(axis=0) / n))
    return dz, (g * xhat).sum(axis=(0, 1)), g.sum(axis=(0, 1))


@pytest.mark.parametrize('c', [32, 96, 512])
@pytest.mark.parametrize('cells', [1, 2, 5])
def test_batch_norm_forward_and_backward(hip_lib, cuda_device, cells, c):
    import torch
    rs = np.random.RandomState(100 * cells + c)
    z = (rs.randn(cells, P, c) * 1.5 + rs.randn(1, 1, c)).astype(f32)
    gamma = (rs.uniform(0.5, 1.5, c) * rs.choice([-1, 1], c)).astype(f32)
    beta = rs.uniform(-0.3, 0.3, c).astype(f32)
    dy = rs.randn(cells, P, c).astype(f32)
    zd, gd, bd, dyd = (dev_of(a, cuda_device) for a in (z, gamma, beta, dy))
    y = torch.full((cells, P, c), float('nan'), device=cuda_device)
    mean, var = torch.full((P, c), float('nan'), device=cuda_device), torch.full((P, c), float('nan'), device=cuda_device)
    assert hip_lib.lrg_pointnet_bn_forward(ptr(zd), ptr(gd), ptr(bd), cells, c, ptr(y), ptr(mean), ptr(var), stream()) == 0
    y, mean, var = y.cpu().numpy(), mean.cpu().numpy(), var.cpu().numpy()
    # moments: a float32 two-pass sum in ascending cell order, bit for bit
    s = np.zeros((P, c), f32)
    for k in range(cells):
        s = s + z[k]
    mu = s / f32(cells)
    q = np.zeros((P, c), f32)
    for k in range(cells):
        d = z[k] - mu
        q = q + d * d
    v = q / f32(cells)
    assert np.array_equal(bits(mean), bits(mu)) and np.array_equal(bits(var), bits(v))
    if cells == 1:
        assert not var.any()

    def normed(dtype):
        zz = z.astype(dtype)
        m_, v_ = zz.mean(axis=0), zz.var(axis=0)
        inv = (dtype(1) / np.sqrt(v_ + dtype(1e-3))) * gamma.astype(dtype)
        return np.maximum(zz * inv + (beta.astype(dtype) - m_ * inv), dtype(0))
    within('y', y, normed(np.float64), normed(np.float32))
    # backward on the kernel's own y, mean and var
    nbytes = hip_lib.lrg_pointnet_bn_backward_workspace_bytes(c)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=cuda_device)
    dz = torch.full((cells, P, c), float('nan'), device=cuda_device)
    dgamma, dbeta = torch.full((c,), float('nan'), device=cuda_device), torch.full((c,), float('nan'), device=cuda_device)
    yd, md, vd = (dev_of(a, cuda_device) for a in (y, mean, var))
    assert hip_lib.lrg_pointnet_bn_backward(ptr(zd), ptr(yd), ptr(dyd), ptr(md), ptr(vd), ptr(gd), cells, c, ptr(dz), ptr(dgamma), ptr(dbeta),
                                            ptr(ws), nbytes, stream()) == 0
    want64, want32 = bn_backward_np(z, y, dy, mean, var, gamma, np.float64), bn_backward_np(z, y, dy, mean, var, gamma, np.float32)
    dz_h = dz.cpu().numpy()
    if cells == 1:
        assert not bits(dz_h).any(), 'a batch of one cell: dz must be +0 everywhere'
        assert not want64[0].any()
    else:
        within('dz', dz_h, want64[0], want32[0])
    within('dgamma', dgamma.cpu().numpy(), want64[1], want32[1])
    within('dbeta', dbeta.cpu().numpy(), want64[2], want32[2])
    # in place (dz = dy) gives the same bits
    assert hip_lib.lrg_pointnet_bn_backward(ptr(zd), ptr(yd), ptr(dyd), ptr(md), ptr(vd), ptr(gd), cells, c, ptr(dyd), ptr(dgamma), ptr(dbeta),
                                            ptr(ws), nbytes, stream()) == 0
    assert np.array_equal(bits(dyd.cpu().numpy()), bits(dz_h))


# ---------------------------------------------------------------- softmax loss ----------------------------------------------------------------
def softmax_np(logits, labels, dtype):
    l = logits.astype(dtype)
    ok = (labels >= 0) & (labels < l.shape[1])
    lab = np.where(ok, labels, 0)
    m = l.max(axis=1, keepdims=True)
    e = np.exp(l - m)
    s = e.sum(axis=1, keepdims=True)
    d = e / s
    d[np.arange(len(l)), lab] -= dtype(1)
    d = d / dtype(len(l))
    d[~ok] = 0
    loss = (np.log(s[:, 0]) + m[:, 0] - l[np.arange(len(l)), lab])[ok].sum()
    return d, float(loss)


@pytest.mark.parametrize('rows', [1, 1024, 3000])
@pytest.mark.parametrize('classes', [1, 2, 13, 41, 260])
def test_softmax_loss(hip_lib, cuda_device, classes, rows):
    import torch
    rs = np.random.RandomState(classes * 7 + rows)
    logits = (rs.randn(rows, classes) * 3).astype(f32)
    labels = rs.randint(0, classes, rows).astype(np.int32)
    logits[0] = f32(1.25)                                  # all equal: the argmax is class 0
    labels[0] = 0
    bad = 0
    if rows >= 3:
        labels[1], labels[2], bad = -1, classes, 2
    ld, yd = dev_of(logits, cuda_device), dev_of(labels, cuda_device)
    d = torch.full((rows, classes), float('nan'), device=cuda_device)
    stats = torch.zeros(3, dtype=torch.float64, device=cuda_device)
    assert hip_lib.lrg_pointnet_softmax_ce_grad(ptr(ld), ptr(yd), rows, classes, ptr(d), ptr(stats), stream()) == 0
    got, s = d.cpu().numpy(), stats.cpu().numpy()
    d64, loss64 = softmax_np(logits, labels, np.float64)
    d32, _ = softmax_np(logits, labels, np.float32)
    within('dlogits', got, d64, d32, scale=1.0 / rows)
    if bad:
        assert not bits(got[1:3]).any()
    np.testing.assert_allclose(s[0], loss64, rtol=2e-5, atol=1e-30)
    ok = (labels >= 0) & (labels < classes)
    assert s[1] == float(((logits.argmax(axis=1) == labels) & ok).sum()) and s[1] >= 1          # row 0 counts: the tie goes to class 0
    assert s[2] == bad
    # accumulated, in a fixed order: a second call (loss only) adds the same bits
    assert hip_lib.lrg_pointnet_softmax_ce_grad(ptr(ld), ptr(yd), rows, classes, None, ptr(stats), stream()) == 0
    s2 = stats.cpu().numpy()
    assert s2[0] == s[0] + s[0] and s2[1] == 2 * s[1] and s2[2] == 2 * bad


# ---------------------------------------------------------------- the head's input ----------------------------------------------------------------
@pytest.mark.parametrize('c_last', [32, 1024])
def test_head_input_and_its_backward(hip_lib, cuda_device, c_last):
    import torch
    cells = 2
    rs = np.random.RandomState(c_last)
    last = np.maximum(rs.randn(cells, P, c_last), 0).astype(f32)
    last[1, :, 5] = 0                                       # a dead channel in one cell: every row ties at zero
    top = last[0].max(axis=0) + f32(1)
    last[0, 3] = top
    last[0, 700] = top                                      # rows 3 and 700 identical and maximal
    pooled = last.max(axis=1)
    dt = rs.randn(cells, P, c_last).astype(f32)
    add = rs.randn(cells, P, c_last).astype(f32)
    ld, pd, dd, ad = (dev_of(a, cuda_device) for a in (last, pooled, dt, add))
    t = torch.full((cells, P, c_last), float('nan'), device=cuda_device)
    assert hip_lib.lrg_pointnet_head_input(ptr(ld), ptr(pd), cells, c_last, ptr(t), stream()) == 0
    assert np.array_equal(bits(t.cpu().numpy()), bits(last - pooled[:, None, :]))
    out = torch.full((cells, P, c_last), float('nan'), device=cuda_device)
    assert hip_lib.lrg_pointnet_head_input_backward(ptr(ld), ptr(pd), ptr(dd), None, cells, c_last, 0, ptr(out), stream()) == 0
    got = out.cpu().numpy()
    win = ref.pool_winner(last, pooled)
    assert (win[0] == 3).all() and win[1, 5] == 0
    S64, S32 = dt.astype(np.float64).sum(axis=1), dt.sum(axis=1, dtype=f32)
    mask = np.zeros(last.shape, bool)
    bi, ci = np.meshgrid(np.arange(cells), np.arange(c_last), indexing='ij')
    mask[bi, win, ci] = True
    assert np.array_equal(bits(got[~mask]), bits(dt[~mask])), 'only the winning row may change'
    assert np.array_equal(bits(got[0, 700]), bits(dt[0, 700]))
    within('winner rows', got[bi, win, ci], dt[bi, win, ci] - S64, dt[bi, win, ci] - S32, scale=float(np.abs(S64).max()))
    # the column sums of a cell: sum(dlast) = S - S
    resid = got.astype(np.float64).sum(axis=1)
    assert np.abs(resid).max() <= max(8 * np.abs(S32 - S64).max(), 2e-5 * np.abs(S64).max())
    # with the skip's gradient added and the ReLU applied, in place
    assert hip_lib.lrg_pointnet_head_input_backward(ptr(ld), ptr(pd), ptr(dd), ptr(ad), cells, c_last, 1, ptr(dd), stream()) == 0
    want = np.where(last > 0, got + add, f32(0))
    assert np.array_equal(bits(dd.cpu().numpy()), bits(want))


@pytest.mark.parametrize('trans', [0, 1])
def test_split_product_stores_its_slices_side_by_side(hip_lib, cuda_device, trans):
    """lrg_gemm_f32_planes: 1000 rows of the reduction in 7 slices (5 chunks of 32 rows each, the last slice short); every plane is
    the product of its own rows, their sum the whole product; a second call gives the same bits."""
    import torch
    M, N, K, split = 70, 40, 1000, 7
    rs = np.random.RandomState(trans)
    A, B = rs.randn(K, M).astype(f32), rs.randn(K, N).astype(f32)
    planes = hip_lib.lrg_gemm_f32_planes_count(K, split)
    assert planes == 7 and hip_lib.lrg_gemm_f32_planes_count(K, 1) == 1 and hip_lib.lrg_gemm_f32_planes_count(64, 5) == 2
    Ad = dev_of(A if trans else np.ascontiguousarray(A.T), cuda_device)
    Bd = dev_of(B, cuda_device)
    outs = []
    for _ in range(2):
        out = torch.full((planes + 1, M, N), float('nan'), device=cuda_device)
        assert hip_lib.lrg_gemm_f32_planes(M, N, K, ptr(Ad), M if trans else K, trans, ptr(Bd), N, 0, ptr(out), split, stream()) == 0
        outs.append(out.cpu().numpy())
    assert np.array_equal(bits(outs[0][:planes]), bits(outs[1][:planes])) and np.isnan(outs[0][planes]).all()
    per = 160                                               # ceil(32 chunks / 7) = 5 chunks of 32 rows
    for z in range(planes):
        a, b = A[z * per:(z + 1) * per], B[z * per:(z + 1) * per]
        within('plane %d' % z, outs[0][z], a.astype(np.float64).T @ b.astype(np.float64), a.T @ b)
    total = torch.empty((M, N), device=cuda_device)
    assert hip_lib.lrg_segment_colsum(ptr(dev_of(outs[0][:planes], cuda_device)), 1, planes, M * N, ptr(total), stream()) == 0
    within('sum', total.cpu().numpy(), A.astype(np.float64).T @ B.astype(np.float64), A.T @ B)
    assert hip_lib.lrg_gemm_f32_planes(M, N, K, None, K, 0, ptr(Bd), N, 0, ptr(out), split, stream()) == EINVAL - 1
    assert hip_lib.lrg_gemm_f32_planes(M, N, K, ptr(Ad), K, 0, ptr(Bd), N, 0, ptr(out), 0, stream()) == EINVAL - 1


def test_bad_arguments(hip_lib, cuda_device):
    import torch
    a = torch.zeros(2 * P * 64, dtype=torch.float32, device=cuda_device)
    i = torch.zeros(16, dtype=torch.int32, device=cuda_device)
    d = torch.zeros(3, dtype=torch.float64, device=cuda_device)
    L, st, p = hip_lib, stream(), ptr(a)
    assert L.lrg_pointnet_bn_forward(None, p, p, 1, 32, p, p, p, st) == EINVAL - 1
    assert L.lrg_pointnet_bn_forward(p, p, p, 0, 32, p, p, p, st) == EINVAL - 2
    assert L.lrg_pointnet_bn_forward(p, p, p, 1, 48, p, p, p, st) == EINVAL - 2
    assert L.lrg_pointnet_bn_forward(p, p, p, 1, 544, p, p, p, st) == EINVAL - 2
    assert L.lrg_pointnet_bn_backward(p, p, p, p, p, p, 1, 32, p, p, None, p, 1 << 20, st) == EINVAL - 1
    assert L.lrg_pointnet_bn_backward(p, p, p, p, p, p, 1, 40, p, p, p, p, 1 << 20, st) == EINVAL - 2
    assert L.lrg_pointnet_bn_backward(p, p, p, p, p, p, 1, 32, p, p, p, p, 2 * P * 32 * 4 - 1, st) == EINVAL - 3
    assert L.lrg_pointnet_softmax_ce_grad(p, None, 4, 2, p, ptr(d), st) == EINVAL - 1
    assert L.lrg_pointnet_softmax_ce_grad(p, ptr(i), 0, 2, p, ptr(d), st) == EINVAL - 2
    assert L.lrg_pointnet_softmax_ce_grad(p, ptr(i), 4, 0, p, ptr(d), st) == EINVAL - 3
    assert L.lrg_pointnet_softmax_ce_grad(p, ptr(i), 4, 1025, p, ptr(d), st) == EINVAL - 3
    assert L.lrg_pointnet_head_input(p, None, 1, 32, p, st) == EINVAL - 1
    assert L.lrg_pointnet_head_input(p, p, 1, 40, p, st) == EINVAL - 2
    assert L.lrg_pointnet_head_input(p, p, 0, 32, p, st) == EINVAL - 2
    assert L.lrg_pointnet_head_input_backward(p, p, None, None, 1, 32, 0, p, st) == EINVAL - 1
    assert L.lrg_pointnet_head_input_backward(p, p, p, None, 70000, 32, 0, p, st) == EINVAL - 2
    assert L.lrg_pointnet_head_input_backward(p, p, p, None, 1, 2048, 0, p, st) == EINVAL - 2
    assert L.lrg_pointnet_ema_update(None, p, 4, 0.1, st) == EINVAL - 1
    assert L.lrg_pointnet_ema_update(p, p, 0, 0.1, st) == EINVAL - 2
    torch.cuda.synchronize()
    assert not a.any() and not d.any()


# ---------------------------------------------------------------- the trainer ----------------------------------------------------------------
TRAINER_CASES = {'tiny-3': ((32, 32), (32,), 3, 3), 'shipped-13': (*pointnet_ref.SHIPPED, 13, 2), 'today-13': (*pointnet_ref.CURRENT, 13, 2),
                 'today-41': (*pointnet_ref.CURRENT, 41, 2)}
_cases = {}


def trainer_case(name):
    """Weights, a batch and the restatement's answers (float64 and float32), computed once per case and left unchanged."""
    if name in _cases:
        return _cases[name]
    conv, fc, ncls, B = TRAINER_CASES[name]
    seed = sorted(TRAINER_CASES).index(name)
    w = ref.init_like(20 + seed, conv, fc, ncls)
    dead = np.arange(conv[0]) % 3 == 0                      # a third of conv0's channels never fire
    w['kernel0'][..., dead] = 0
    w['bias0'][dead] = f32(-0.1)
    rs = np.random.RandomState(40 + seed)
    pts = rs.uniform(-1, 1, (B, P, 6)).astype(f32)
    pts[:, :, 2] = rs.uniform(0, 2.5, (B, P))
    lab = rs.randint(0, ncls, (B, P))
    pts[:, 900] = pts[:, 17]                                # a cell drawn with replacement holds one point twice
    lab[:, 900] = lab[:, 17]
    fw64, g64 = ref.loss_and_grads(pts, lab, w, np.float64)
    fw32, g32 = ref.loss_and_grads(pts, lab, w, np.float32)
    _cases[name] = dict(w=w, pts=pts, lab=lab, fw=fw64, fw32=fw32, G=g64, G32=g32, conv=conv, fc=fc, ncls=ncls, B=B)
    return _cases[name]


def make_trainer(case, dev, **kw):
    from learn_region_grow_amd.pointnet_train import PointNetTrainer
    return PointNetTrainer(case['B'], case['conv'], case['fc'], case['ncls'], device=dev, **kw).load_weights(case['w'])


@pytest.mark.parametrize('name', sorted(TRAINER_CASES))
def test_backward_matches_the_restatement(cuda_device, name):
    """Loss (rtol 2e-5), accuracy and every gradient.  A hidden fc_bias has a zero gradient in exact arithmetic (the batch norm
    removes the batch mean), so its bound takes `scale` from that block's beta gradient.  The accuracy may differ by the rows whose
    two largest float64 logits are closer than 1e-4 of the largest logit: float32 logits cannot reorder any other row."""
    case = trainer_case(name)
    tr = make_trainer(case, cuda_device)
    tr.gflat.fill_(float('nan'))
    sc = tr.backward(case['pts'], case['lab'])
    fw = case['fw']
    print('loss %.6f (restatement %.6f)  acc %.4f (%.4f)' % (sc['loss'], fw['loss'], sc['acc'], fw['acc']))
    np.testing.assert_allclose(sc['loss'], fw['loss'], rtol=2e-5)
    top = np.sort(fw['logits'], axis=2)
    close = int(((top[..., -1] - top[..., -2]) < 1e-4 * np.abs(fw['logits']).max()).sum()) if case['ncls'] > 1 else 0
    assert abs(sc['acc'] - fw['acc']) * case['B'] * P <= close + 1e-6
    got = tr.grads_numpy()
    assert sorted(got) == sorted(ref.trainable_names(case['conv'], case['fc']))
    for k in sorted(got):
        scale = None
        if k.startswith('fc_bias') and k != 'fc_bias%d' % len(case['fc']):
            scale = float(np.abs(case['G'][ref.bn_names(int(k[len('fc_bias'):]))[0]]).max())
        within(k, got[k], case['G'][k], case['G32'][k], scale)
    # the batch's moments
    mom = tr.moments_numpy()
    for j in range(len(case['fc'])):
        within('mean %d' % j, mom[ref.bn_names(j)[2]], fw['means'][j], case['fw32']['means'][j])
        within('variance %d' % j, mom[ref.bn_names(j)[3]], fw['variances'][j], case['fw32']['variances'][j])
    # evaluate-style call: loss only, nothing else touched
    tr.gflat.fill_(-777.25)
    assert tr.backward(case['pts'], case['lab'], loss_only=True) == sc
    assert (tr.gflat == -777.25).all()


def test_labels_out_of_range_raise(cuda_device):
    case = trainer_case('tiny-3')
    tr = make_trainer(case, cuda_device)
    lab = case['lab'].copy()
    lab[1, 7] = 3
    with pytest.raises(ValueError):
        tr.backward(case['pts'], lab)


@pytest.mark.parametrize('name', ['tiny-3', 'shipped-13'])
def test_train_step_is_adam_at_the_scheduled_rate_on_the_trainers_own_gradients(cuda_device, name):
    """Three steps with decay_steps = 2, so that the rate halves before the third: after each, the flat weights, m and v carry the
    bits of the float32 restatement of Adam applied to the trainer's own gradients; after the first the moving averages are
    float32(1 - 0.9) * the batch's moments, bit for bit, and after each the script's update of them."""
    case = trainer_case(name)
    tr = make_trainer(case, cuda_device, decay_steps=2)
    flat = lambda d: np.concatenate([d[k].reshape(-1) for k in tr.names])
    w0 = tr.weights_numpy()
    p, m, v = flat(w0), np.zeros(tr.flat.numel(), f32), np.zeros(tr.flat.numel(), f32)
    shadow = {k: w0[k] for k in tr.ema_views}
    assert all(not s.any() for s in shadow.values())
    for step in range(3):
        assert tr.step == step
        lr = 2e-4 * 0.5 ** (step // 2)
        assert tr.learning_rate() == lr
        tr.train_step(case['pts'], case['lab'])
        g, t = flat(tr.grads_numpy()), step + 1
        p, m, v = adam_f32(p, g, m, v, lr * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t), 0.9, 0.999, 1e-8)
        for what, got, want in (('weights', tr.flat, p), ('m', tr.m, m), ('v', tr.v, v)):
            bad = bits(got.cpu().numpy()) != bits(want)
            assert not bad.any(), 'step %d %s: %d of %d differ' % (step, what, bad.sum(), bad.size)
        mom, now = tr.moments_numpy(), tr.weights_numpy()
        for k in shadow:
            if step == 0:
                assert np.array_equal(bits(now[k]), bits(f32(1 - 0.9) * mom[k]))
            shadow[k] = ref.ema_update(shadow[k], mom[k])
            assert np.array_equal(bits(now[k]), bits(shadow[k])), k
    assert tr.step == 3


def test_three_steps_twice_give_the_same_bits(cuda_device):
    case = trainer_case('shipped-13')
    runs = []
    for _ in range(2):
        tr = make_trainer(case, cuda_device)
        rs = np.random.RandomState(3)
        for step in range(3):
            tr.train_step(case['pts'] + rs.uniform(-0.01, 0.01, case['pts'].shape).astype(f32), case['lab'])
        runs.append([bits(t.cpu().numpy()) for t in (tr.flat, tr.m, tr.v, tr.ema, tr.gflat)])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def band_batch(step, B=2, ncls=3):
    """The class of a point is its height band: 0 .. 1 m, 1 .. 2 m, 2 .. 3 m."""
    rs = np.random.RandomState(1000 + step)
    p = rs.uniform(-0.5, 0.5, (B, P, 6)).astype(f32)
    p[:, :, 2] = rs.uniform(0, 3, (B, P))
    return p, np.minimum(p[:, :, 2].astype(int), ncls - 1)


def test_it_learns(cuda_device):
    """20 steps at a base rate of 1e-2 on the tiny network: the float64 restatement's loss falls by more than a quarter (1.32 ->
    0.55 on the CPU); the GPU trainer's must fall by at least half of that drop."""
    from learn_region_grow_amd.pointnet_train import PointNetTrainer, initial_weights
    conv, fc, ncls, steps = (32, 32), (32,), 3, 20
    w = initial_weights(conv, fc, ncls, seed=0)
    _, want = ref.train(band_batch, w, steps, base=1e-2)
    drop = want[0] - want[-1]
    assert drop >= 0.25 * want[0]
    tr = PointNetTrainer(2, conv, fc, ncls, device=cuda_device, base_learning_rate=1e-2).load_weights(w)
    got = [tr.train_step(*band_batch(s))['loss'] for s in range(steps)]
    print('restatement %.4f -> %.4f, trainer %.4f -> %.4f' % (want[0], want[-1], got[0], got[-1]))
    np.testing.assert_allclose(got[0], want[0], rtol=2e-5)
    assert got[0] - got[-1] >= 0.5 * drop


def test_save_load_and_inference_round_trip(cuda_device, tmp_path):
    import torch
    from learn_region_grow_amd import checkpoint
    from learn_region_grow_amd.pointnet import PointNetHIP
    case = trainer_case('shipped-13')
    tr = make_trainer(case, cuda_device)
    for _ in range(3):
        tr.train_step(case['pts'], case['lab'])
    ev = tr.evaluate(case['pts'], case['lab'])
    behind = tr.eval_logits(case['pts']).cpu().numpy()
    prefix = str(tmp_path / 'models' / 'pointnet_model5.ckpt')
    tr.save(prefix)
    back = checkpoint.load_pointnet_weights(prefix)
    now = tr.weights_numpy()
    assert all(np.array_equal(bits(back[k]), bits(now[k])) for k in now)
    everything = checkpoint.load_bundle(prefix)
    assert int(everything['Variable']) == 3 and everything['kernel0/Adam'].any() and 'beta2_power' in everything
    logits = PointNetHIP(back, device=cuda_device).logits(case['pts'])
    assert np.array_equal(bits(logits), bits(behind))
    # the loss and accuracy behind evaluate() are those of these logits
    d64, loss64 = softmax_np(logits.reshape(-1, 13), case['lab'].reshape(-1).astype(np.int32), np.float64)
    np.testing.assert_allclose(ev['loss'], loss64 / logits[..., 0].size, rtol=2e-5)
    assert ev['acc'] == float((logits.argmax(axis=2) == case['lab']).mean())
    torch.cuda.synchronize()


def test_command_line_trains_and_the_checkpoint_runs(cuda_device, tmp_path):
    from learn_region_grow_amd import checkpoint, io, synthetic
    raw = [synthetic.area5_shaped_room(2500, 11).astype(f32), synthetic.area5_shaped_room(1800, 12).astype(f32)]
    data = tmp_path / 'data'
    data.mkdir()
    h5 = str(data / 's3dis_area1.h5')
    io.saveToH5(h5, raw)
    p = subprocess.run([sys.executable, os.path.join(REPO, 'train_pointnet.py'), '--mode', 'pointnet', '--train-area', '1', '--val-area', '1',
                        '--data-dir', str(data), '--model-dir', str(tmp_path / 'models'), '--epochs', '1', '--val-step', '1', '--batch-size', '2',
                        '--arch', 'shipped'], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.split('\n')
    assert any(l.startswith('Epoch: 0 Loss: ') and '(cls ' in l for l in lines), p.stdout[-2000:]
    assert any(l.startswith('Validation: 0 Loss: ') for l in lines), p.stdout[-2000:]
    ck = str(tmp_path / 'models' / 'pointnet_model1.ckpt')
    w = checkpoint.load_pointnet_weights(ck)
    assert checkpoint.pointnet_variant({k: v.shape for k, v in w.items()}) == (*pointnet_ref.SHIPPED, 13)
    assert int(checkpoint.load_bundle(ck, names=['Variable'])['Variable']) >= 1
    p = subprocess.run([sys.executable, os.path.join(REPO, 'pointnet.py'), '--h5', h5, '--area', '1', '--ckpt', ck], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    assert 'Restored from %s' % ck in p.stdout
