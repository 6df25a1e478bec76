"""GPU: the training kernels of csrc/lrg_train.hip one by one (lrg_ce_grad, lrg_pool_backward, lrg_segment_colsum, lrg_adam_step,
lrg_gemm_f32) against plain NumPy, and the trainer (learn_region_grow_amd.train.LrgNetTrainer) against the float64 oracle
(oracle/train_ref.py) at the shapes where its host sequencing takes another path: a split dW reduction, Ni != Nn, B = 1, an empty
remove class, evaluate(), Adam on its own gradients.

Every tolerance here is bit equality, a bound derived in the docstring from EPS = 2^-24 (the unit roundoff of float32) and a count
of the operations, or the stated multiple of the float32 oracle's own error.  The library is built with -ffp-contract=off and
without fast-math, and hipcc rounds float32 division and square root correctly by default, so + - * / sqrt in a kernel round
like NumPy's float32."""
import ctypes
import functools

import numpy as np
import pytest

from learn_region_grow_amd import synthetic
from oracle import lrgnet_ref, train_ref
from test_gpu_train import WEIGHT_KW

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
EINVAL = -1000
f32 = np.float32


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _at(t, elements):
    """Pointer `elements` float32 elements into tensor t."""
    return ctypes.c_void_p(t.data_ptr() + 4 * elements)


# ---------------------------------------------------------------- 1. lrg_ce_grad ----------------------------------------------------------------
def _ce_block():
    """The constructed logit pairs, each once under label 0 and once under a non-zero label (1 and 7 alternate)."""
    up = lambda x: np.nextafter(f32(x), f32(np.inf))
    pairs = [(0, 0), (1.5, 1.5), (-7, -7), (3e4, 3e4),                                  # ties: class 0 is predicted
             (80, -80), (-80, 80), (3e4, -3e4), (-3e4, 3e4),                            # exp underflows: the loss term is m - l_y
             (1.0, up(1.0)), (up(1.0), 1.0), (-2.5, up(-2.5)), (up(-2.5), -2.5)]        # differ in the last bit
    lg = np.array(pairs + pairs, dtype=np.float32)
    lab = np.array([0] * len(pairs) + [1, 7] * (len(pairs) // 2), dtype=np.int32)
    return lg, lab


def _ce_inputs(rows):
    rs = np.random.RandomState(rows)
    lg = (rs.randn(rows, 2) * 3).astype(np.float32)
    lab = rs.choice([0, 1, 7], rows).astype(np.int32)
    blg, blab = _ce_block()
    k = min(rows, len(blg))
    lg[:k], lab[:k] = blg[:k], blab[:k]
    for start in (1024 * 256 + 5, rows - len(blg)):                # past the grid's first sweep, and the very last rows
        if 1024 * 256 <= start <= rows - len(blg):
            lg[start:start + len(blg)], lab[start:start + len(blg)] = blg, blab
    return lg, lab


def _ce_weights(kind, lab):
    n_pos = int((lab != 0).sum())
    n_neg = lab.size - n_pos
    inv = lambda n: 1.0 / n if n else 0.0                            # an empty class contributes nothing (train.py)
    return {'mean': (1.0 / lab.size, 1.0 / lab.size), 'per_class': (inv(n_pos), inv(n_neg)), 'neg_only': (0.0, inv(n_neg)),
            'pos_only': (inv(n_pos), 0.0)}[kind]


@pytest.mark.parametrize('kind', ['mean', 'per_class', 'neg_only', 'pos_only'])
@pytest.mark.parametrize('rows', [1, 255, 257, 300001])
def test_ce_grad_against_float64(cuda_device, hip_lib, rows, kind):
    """dlogits, the weighted loss and the five counters of lrg_ce_grad; a second call accumulates.

    Counters: integers, exact.  The prediction is l1 > l0 (a tie predicts class 0, as tf.argmax does), the label is labels != 0.

    dlogits, per row, with u = EPS and every float32 operation correctly rounded (relative error <= u); expf and logf are allowed
    2 ulp = 4u relative each: no ulp table of the device library is installed next to this toolchain to take a figure from.  m = max(l0, l1) is exact, so one exponent argument is exactly 0
    and its e = 1 exactly.  For the other, d = fl(l - m) = d*(1 + u) <= 0 and e = exp(d) in [0, 1]:
      |e^ - e| <= e|d|u + 4u e <= (1/e + 4)u = 4.37u            (x exp(-x) <= 1/e; an underflowing e errs by < 2^-126)
      s = fl(1 + e^) in [1, 2], p = fl(e_i / s): both p are functions of e with |dp/de| <= 1, plus 2 roundings of relative u:
      |p^small - p| <= 4.37u + 2u*0.5 = 5.37u,   |p^big - p| <= 4.37u + 2u = 6.37u
      p - onehot: p - 0 and p_big - 1 are exact (Sterbenz); p_small - 1 rounds once, <= u           -> 7.37u
      times w (w is the float32 the kernel was given): one rounding of a value of magnitude <= w    -> (7.37 + 1)u w
    so |dlogits^ - dlogits| <= 9 u w.

    Loss, per row t = w (log s + m - l_y), ce = log s + m - l_y >= 0:
      s^ errs by 4.37u + u s <= 6.37u absolutely, log' <= 1 on [1, 2]; logf adds 4u log 2 = 2.78u           -> 9.15u
      fl(L + m) adds u(|m| + log 2), fl(. - l_y) adds u ce, the product with w adds u w ce
    so |t^ - t| <= u w (10 + |m| + 2 ce).  The terms are then summed in float64 (relative error ~rows * 2^-53, absorbed by the
    rounding of 9.85 up to 10), which gives |loss^ - loss| <= u * sum_r w_r (10 + |m_r| + 2 ce_r)."""
    import torch
    from learn_region_grow_amd.lrgnet import _ptr, _stream_ptr
    lg, lab = _ce_inputs(rows)
    w_pos, w_neg = (float(f32(x)) for x in _ce_weights(kind, lab))
    y = lab != 0
    l64 = lg.astype(np.float64)
    m = l64.max(axis=1)
    e = np.exp(l64 - m[:, None])
    p = e / e.sum(axis=1, keepdims=True)
    ce = np.log(e.sum(axis=1)) + m - np.where(y, l64[:, 1], l64[:, 0])
    w = np.where(y, w_pos, w_neg)
    want = (p - np.stack([~y, y], axis=1)) * w[:, None]
    pred = lg[:, 1] > lg[:, 0]
    counts = np.array([(pred == y).sum(), (pred & y).sum(), pred.sum(), y.sum(), rows], dtype=np.float64)
    loss, loss_tol = float((w * ce).sum()), float(EPS * (w * (10 + np.abs(m) + 2 * ce)).sum())

    dlg, dlab = _dev(lg, cuda_device), _dev(lab, cuda_device)
    dl = torch.full((rows, 2), float('nan'), dtype=torch.float32, device=cuda_device)
    stats = torch.zeros(8, dtype=torch.float64, device=cuda_device)
    for call in (1, 2):
        assert hip_lib.lrg_ce_grad(_ptr(dlg), _ptr(dlab), rows, w_pos, w_neg, _ptr(dl), _ptr(stats), _stream_ptr()) == 0
        s = stats.cpu().numpy()
        got = dl.cpu().numpy().astype(np.float64)
        err = np.abs(got - want) / np.maximum(w, 1e-300)[:, None]
        print('call %d: dlogits err %.2f u w (bound 9), loss err %.3e (bound %.3e)' %
              (call, float(np.where(w[:, None] > 0, err, 0).max() / EPS), abs(s[0] - call * loss), call * loss_tol))
        assert np.array_equal(s[1:6], call * counts), (s[1:6], counts)
        assert np.array_equal(s[6:], [0, 0])
        assert (np.abs(got - want) <= 9 * EPS * w[:, None]).all()
        assert abs(s[0] - call * loss) <= call * loss_tol


def test_ce_grad_rejects_bad_arguments(cuda_device, hip_lib):
    import torch
    from learn_region_grow_amd.lrgnet import _ptr, _stream_ptr
    lg, lab = _dev(np.ones((4, 2), np.float32), cuda_device), _dev(np.ones(4, np.int32), cuda_device)
    dl = torch.full((4, 2), -3.0, dtype=torch.float32, device=cuda_device)
    stats = torch.full((8,), -3.0, dtype=torch.float64, device=cuda_device)
    good = [_ptr(lg), _ptr(lab), 4, 0.25, 0.25, _ptr(dl), _ptr(stats)]
    for pos, bad in [(0, None), (1, None), (5, None), (6, None), (2, 0), (2, -1)]:
        args = list(good)
        args[pos] = bad
        assert hip_lib.lrg_ce_grad(*args, _stream_ptr()) == EINVAL - 1, pos
    torch.cuda.synchronize()
    assert (dl == -3.0).all() and (stats == -3.0).all()


# ------------------------------------------------------------- 2. lrg_pool_backward -------------------------------------------------------------
def _pool_inputs(B, rows, C, seed):
    """Post-ReLU y [B,rows,C] whose leading columns are constructed (as far as rows and C allow), the rest max(randn, 0)."""
    rs = np.random.RandomState(seed)
    y = np.maximum(rs.randn(B, rows, C), 0).astype(np.float32)
    def first_row(col): col[0] = 9.0                                                    # unique maximum in the first row
    def last_row(col): col[rows - 1] = 9.0                                              # ... in the last row
    def two_rows(col): col[[0, rows - 1]] = 9.0                                         # shared by 2 rows
    def three_rows(col): col[[0, rows // 2, rows - 1]] = 9.0                            # shared by 3 rows
    def all_rows(col): col[:] = 0.75                                                    # shared by all rows (a padded set)
    def all_zero(col): col[:] = 0.0                                                     # all zero: passes nothing
    def denormal(col):
        col[:] = 0.0
        col[rows // 3] = 1e-40                                                          # the only positive entry is denormal
    cols = [first_row, last_row, two_rows, three_rows, all_rows, all_zero, denormal]
    for b in range(B):
        for c, make in enumerate(cols[:C]):
            make(y[b, :, (c + b) % C])                                                  # another column per instance
    return y


@pytest.mark.parametrize('B,rows,C,stride,off', [(1, 1, 1, 1, 0), (2, 64, 512, 1024, 0), (2, 64, 512, 1024, 512), (3, 37, 257, 300, 0),
                                                 (2, 128, 64, 64, 0)])
def test_pool_backward_bit_exact(cuda_device, hip_lib, B, rows, C, stride, off):
    """dy = where(y == colmax and colmax > 0, float32(dpool) / float32(ties), 0): the only arithmetic is one correctly rounded
    division, so the bits are compared.  dy starts as NaN: an element the kernel does not write fails."""
    import torch
    from learn_region_grow_amd.lrgnet import _ptr, _stream_ptr
    y = _pool_inputs(B, rows, C, seed=rows + C)
    dpool = np.random.RandomState(C).randn(B, stride).astype(np.float32)
    dpool[dpool == 0] = 1.0
    mx = y.max(axis=1, keepdims=True)
    tie = y == mx
    g = dpool[:, None, off:off + C] / tie.sum(axis=1, keepdims=True).astype(np.float32)
    assert g.dtype == np.float32
    want = np.where(tie & (mx > 0), g, f32(0))
    dy = torch.full((B, rows, C), float('nan'), dtype=torch.float32, device=cuda_device)
    dp, dev_y = _dev(dpool, cuda_device), _dev(y, cuda_device)
    assert hip_lib.lrg_pool_backward(_ptr(dev_y), _at(dp, off), B, rows, C, stride, _ptr(dy), _stream_ptr()) == 0
    got = dy.cpu().numpy()
    bad = _bits(got) != _bits(want)
    assert not bad.any(), 'first of %d: %s got %r want %r' % (bad.sum(), np.argwhere(bad)[0], got[bad][0], want[bad][0])


def test_pool_backward_rejects_a_short_stride(cuda_device, hip_lib):
    import torch
    from learn_region_grow_amd.lrgnet import _ptr, _stream_ptr
    y = torch.ones((2, 4, 8), dtype=torch.float32, device=cuda_device)
    dy = torch.full((2, 4, 8), -3.0, dtype=torch.float32, device=cuda_device)
    assert hip_lib.lrg_pool_backward(_ptr(y), _ptr(y), 2, 4, 8, 7, _ptr(dy), _stream_ptr()) == EINVAL - 1
    torch.cuda.synchronize()
    assert (dy == -3.0).all()


# ------------------------------------------------------------ 3. lrg_segment_colsum ------------------------------------------------------------
@pytest.mark.parametrize('n_seg,seg_rows,N', [(1, 1, 1), (3, 64, 2), (2, 37, 257), (34, 64, 256), (65535, 1, 3)])
def test_segment_colsum(cuda_device, hip_lib, n_seg, seg_rows, N):
    """Integer-valued inputs in [-8, 8] sum exactly in any order: the bits are compared.  randn inputs: a sum of n float32 terms
    in any order is within (n - 1) u sum|x| of the exact one, here asserted as n * EPS * sum|x| with n = seg_rows for one pass,
    and n = seg_rows + n_seg for the trainer's two passes (per-instance partials, then one segment over the partials:
    (seg_rows - 1) + (n_seg - 1) roundings on any path to an output)."""
    import torch
    from learn_region_grow_amd.lrgnet import _ptr, _stream_ptr
    rs = np.random.RandomState(n_seg + N)
    out = torch.empty((n_seg, N), dtype=torch.float32, device=cuda_device)
    tot = torch.empty(N, dtype=torch.float32, device=cuda_device)

    def run(x):
        out.fill_(float('nan'))
        tot.fill_(float('nan'))
        dx = _dev(x, cuda_device)
        assert hip_lib.lrg_segment_colsum(_ptr(dx), n_seg, seg_rows, N, _ptr(out), _stream_ptr()) == 0
        assert hip_lib.lrg_segment_colsum(_ptr(out), 1, n_seg, N, _ptr(tot), _stream_ptr()) == 0
        return out.cpu().numpy(), tot.cpu().numpy()
    xi = rs.randint(-8, 9, (n_seg, seg_rows, N)).astype(np.float32)
    part, total = run(xi)
    assert np.array_equal(_bits(part), _bits(xi.sum(axis=1, dtype=np.float64).astype(np.float32)))
    assert np.array_equal(_bits(total), _bits(xi.sum(axis=(0, 1), dtype=np.float64).astype(np.float32)))
    x = rs.randn(n_seg, seg_rows, N).astype(np.float32)
    part, total = run(x)
    x64 = x.astype(np.float64)
    assert (np.abs(part - x64.sum(axis=1)) <= seg_rows * EPS * np.abs(x64).sum(axis=1)).all()
    assert (np.abs(total - x64.sum(axis=(0, 1))) <= (seg_rows + n_seg) * EPS * np.abs(x64).sum(axis=(0, 1))).all()


def test_segment_colsum_rejects_too_many_segments(cuda_device, hip_lib):
    import torch
    from learn_region_grow_amd.lrgnet import _ptr, _stream_ptr
    x = torch.ones((65536, 1), dtype=torch.float32, device=cuda_device)
    out = torch.full((65536, 1), -3.0, dtype=torch.float32, device=cuda_device)
    assert hip_lib.lrg_segment_colsum(_ptr(x), 65536, 1, 1, _ptr(out), _stream_ptr()) == EINVAL - 1
    torch.cuda.synchronize()
    assert (out == -3.0).all()


# -------------------------------------------------------------- 4. lrg_adam_step --------------------------------------------------------------
def adam_lr_t(lr, b1, b2, t):
    return lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)                                 # train.py: in double, passed as c_float


def adam_f32(p, g, m, v, lr_t, b1, b2, eps):
    """lrg_adam_kernel's expression, operation by operation, in NumPy float32 -> (p, m, v)."""
    lr_t, b1, b2, eps, one = f32(lr_t), f32(b1), f32(b2), f32(eps), f32(1)
    m2 = m + (g - m) * (one - b1)
    v2 = v + (g * g - v) * (one - b2)
    p2 = p - lr_t * m2 / (np.sqrt(v2) + eps)
    assert p2.dtype == m2.dtype == v2.dtype == np.float32
    return p2, m2, v2


def adam_oracle_bounds(p, g, m, v, t, lr, b1, b2, eps):
    """One step of oracle.train_ref.Adam (float64, TensorFlow-1 semantics) from the float32 state (p, m, v) with the float32
    gradient g -> (p*, m*, v*) and the bounds (dp, dm, dv) within which the float32 restatement must stay.

    u = EPS; every float32 operation errs by <= u relative.  The float32 chain uses b' = fl(1) - fl(beta), an exact subtraction
    of a rounded beta: e1 = |b1' - (1 - b1)| / (1 - b1), e2 likewise (about 1.5e-7 and 1.3e-5 for 0.9 and 0.999: the constant of
    the slow average is the worst rounded number of the step).  To first order:
      dm = (e1 + 2u)(1 - b1)|g - m| + u|m*|                          (g - m, its product with b1', the sum)
      dv = (1 - b2)((e2 + 2u)|g g - v| + u g g) + u|v*|               (g g, the difference, the product with b2', the sum)
      ds = dv / sqrt(v*) + u sqrt(v*)                                 (|sqrt a - sqrt b| <= |a - b| / sqrt b; sqrtf rounds once)
      dden = ds + u eps + u den*                                      (eps as float32, the sum)
      dnum = lr_t dm + 2u lr_t |m*|                                   (lr_t as float32, the product)
      dq = dnum / den* + q* dden / den* + u q*                        (the quotient), q* = lr_t |m*| / den* the step
    and p - q rounds once on either side (the oracle returns float32 too), so |p^ - p*| <= dq + one ulp of p.  Relative
    perturbations stay below 1e-4, so the neglected second-order terms are covered by a factor 1 + 2^-10."""
    opt = train_ref.Adam(lr, b1, b2, eps)
    opt.t = t - 1
    opt.m, opt.v = {'x': m.astype(np.float64)}, {'x': v.astype(np.float64)}
    ps = opt.step({'x': p}, {'x': g})['x']
    ms, vs = opt.m['x'], opt.v['x']
    u = EPS
    g, m, v = g.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
    e1 = abs(float(f32(1) - f32(b1)) - (1 - b1)) / (1 - b1)
    e2 = abs(float(f32(1) - f32(b2)) - (1 - b2)) / (1 - b2)
    dm = (e1 + 2 * u) * (1 - b1) * np.abs(g - m) + u * np.abs(ms)
    dv = (1 - b2) * ((e2 + 2 * u) * np.abs(g * g - v) + u * g * g) + u * np.abs(vs)
    sq = np.sqrt(vs)
    ds = np.divide(dv, sq, out=np.zeros_like(sq), where=sq > 0) + u * sq
    den = sq + eps
    lr_t = adam_lr_t(lr, b1, b2, t)
    q = lr_t * np.abs(ms) / den
    dq = (lr_t * dm + 2 * u * lr_t * np.abs(ms)) / den + q * (ds + u * eps + u * den) / den + u * q
    k = 1 + 2.0 ** -10
    return ps, ms, vs, k * dq, k * dm, k * dv


def _adam_state(n, seed):
    """Per-element scales log-uniform over 1e-8 .. 1e3 (sqrt(v) comparable with epsilon at the low end), non-zero m and v of
    matching size; every 16th element is an exact zero with m = v = 0."""
    rs = np.random.RandomState(seed)
    scale = (10.0 ** rs.uniform(-8, 3, n))
    scale[:min(n, 64):2] = 10.0 ** rs.uniform(-8, -5, len(scale[:min(n, 64):2]))          # the low end is always populated
    scale[5::16] = 0.0
    p = rs.randn(n).astype(np.float32)
    m = (0.5 * scale * rs.randn(n)).astype(np.float32)
    v = (scale ** 2 * rs.rand(n)).astype(np.float32)
    return rs, scale, p, m, v


@pytest.mark.parametrize('n', [1, 255, 256, 257, 100003])
def test_adam_step_bit_exact(cuda_device, hip_lib, n):
    """Five steps t = 1..5 from non-zero m, v: p, m and v after every step carry the bits of the float32 restatement, which in
    turn stays within the derived bound (adam_oracle_bounds) of the float64 oracle on every step."""
    from learn_region_grow_amd.lrgnet import _ptr, _stream_ptr
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    rs, scale, p, m, v = _adam_state(n, seed=n)
    zero = scale == 0
    p0 = p.copy()
    dp, dm, dv = (_dev(a, cuda_device) for a in (p, m, v))
    for t in range(1, 6):
        g = (scale * rs.randn(n)).astype(np.float32)
        lr_t = adam_lr_t(lr, b1, b2, t)
        dg = _dev(g, cuda_device)
        assert hip_lib.lrg_adam_step(_ptr(dp), _ptr(dg), _ptr(dm), _ptr(dv), n, ctypes.c_float(lr_t), ctypes.c_float(b1),
                                     ctypes.c_float(b2), ctypes.c_float(eps), _stream_ptr()) == 0
        ps, ms, vs, tp, tm, tv = adam_oracle_bounds(p, g, m, v, t, lr, b1, b2, eps)
        p, m, v = adam_f32(p, g, m, v, lr_t, b1, b2, eps)
        for name, got, want in (('p', dp, p), ('m', dm, m), ('v', dv, v)):
            bad = _bits(got.cpu().numpy()) != _bits(want)
            assert not bad.any(), 't=%d %s: %d of %d differ, first at %d: got %r want %r' % (
                t, name, bad.sum(), n, np.argmax(bad), got.cpu().numpy()[np.argmax(bad)], want[np.argmax(bad)])
        ulp = np.spacing(np.maximum(np.abs(p), np.abs(ps)))
        assert (np.abs(m - ms) <= tm).all() and (np.abs(v - vs) <= tv).all()
        assert (np.abs(p.astype(np.float64) - ps.astype(np.float64)) <= tp + ulp).all()
    assert np.isfinite(p).all() and np.array_equal(p[zero], p0[zero]) and not m[zero].any() and not v[zero].any()
    # the low end is what tells sqrt(v) + eps from sqrt(v + eps): make sure the data has it
    assert ((np.sqrt(v) < 1e3 * eps) & (v > 0)).any()


# --------------------------------------------------------------- 5. lrg_gemm_f32 ---------------------------------------------------------------
def _padded(rs, rows, cols, ld, fill):
    """A [rows, cols] randn matrix inside a [rows + 2, ld] buffer whose padding holds `fill`."""
    buf = np.full((rows + 2, ld), fill, dtype=np.float32)
    buf[:rows, :cols] = rs.randn(rows, cols)
    return buf


GEMM_SHAPES = [(70, 50, 37, 1), (1, 50, 37, 1), (70, 1, 37, 1), (70, 50, 1, 1), (1, 1, 1, 1), (65, 33, 31, 1), (65, 33, 32, 1), (65, 33, 33, 1),
               (33, 65, 40, 5), (33, 65, 20, 3), (64, 64, 100, 3), (13, 70, 70, 2), (5, 3, 900, 4)]


@pytest.mark.parametrize('tA,tB', [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize('M,N,K,split', GEMM_SHAPES)
def test_gemm_layouts_strides_and_splits(cuda_device, hip_lib, M, N, K, split, tA, tB):
    """The four operand layouts; M, N, K of 1; K around the 32-wide chunk; split_k past the number of chunks (K = 40 / 5,
    K = 20 / 3), with a partial last slice (K = 100 / 3: 64 + 36; K = 70 / 2: 64 + 6) and into a non-zero C (the entry point ADDs).
    Each case runs with tight and with padded leading dimensions.  The padding of A, B, addend and mask is NaN (it must never
    reach a product); C's padding columns and the rows past M hold a sentinel and must keep it.

    Tolerance: the textbook bound for a K-term float32 inner product in any order, K * EPS * (|A| |B|) elementwise, times 2 for
    a split: its at most split_k atomic additions each round a running sum no larger than |C_before| + |A| |B|, which stays
    within the second K * EPS * (|A| |B|) as long as split_k (|C_before| + |A| |B|) <= K |A| |B| (asserted of the data).
    The addend adds one rounding of the result, EPS * |result|."""
    from learn_region_grow_amd.lrgnet import _ptr, _stream_ptr
    rs = np.random.RandomState(1000 * M + 10 * K + 2 * tA + tB)
    nan = float('nan')
    for pad in (0, 1):
        ar, ac = (K, M) if tA else (M, K)
        br, bc = (N, K) if tB else (K, N)
        lda, ldb, ldc = ac + 35 * pad, bc + 37 * pad, N + 3 * pad
        A, Bm = _padded(rs, ar, ac, lda, nan), _padded(rs, br, bc, ldb, nan)
        a64, b64 = A[:ar, :ac].astype(np.float64), Bm[:br, :bc].astype(np.float64)
        a64, b64 = (a64.T if tA else a64), (b64.T if tB else b64)
        prod, mag = a64 @ b64, np.abs(a64) @ np.abs(b64)
        C0 = _padded(rs, M, N, ldc, -777.25)
        if split == 1:
            C0[:M, :N] = nan                                            # overwritten, never read
        dA, dB = _dev(A, cuda_device), _dev(Bm, cuda_device)
        variants = [(None, None)]
        if split == 1:
            add, mask = _padded(rs, M, N, ldc, nan), _padded(rs, M, N, ldc, nan)
            variants += [(add, None), (None, mask), (add, mask)]
        for add, mask in variants:
            C = _dev(C0, cuda_device)
            dadd = _dev(add, cuda_device) if add is not None else None                 # named: both live through the call
            dmask = _dev(mask, cuda_device) if mask is not None else None
            rc = hip_lib.lrg_gemm_f32(M, N, K, _ptr(dA), lda, tA, _ptr(dB), ldb, tB, _ptr(C), ldc, _ptr(dadd), _ptr(dmask), split,
                                      _stream_ptr())
            assert rc == 0
            got = C.cpu().numpy()
            if split > 1:
                want = C0[:M, :N].astype(np.float64) + prod
                tol = 2 * K * EPS * mag
                assert (split * (np.abs(C0[:M, :N]) + mag) <= K * mag).all()           # the data keeps the slices' additions within the factor 2
            else:
                want = prod + (add[:M, :N] if add is not None else 0.0)
                tol = K * EPS * mag + (EPS * np.abs(want) if add is not None else 0.0)
                if mask is not None:
                    want, tol = np.where(mask[:M, :N] > 0, want, 0.0), np.where(mask[:M, :N] > 0, tol, 0.0)
            err = np.abs(got[:M, :N] - want)
            assert (err <= tol).all(), 'pad %d addend %s mask %s: worst err / tol %.3g' % (
                pad, add is not None, mask is not None, float((err / np.maximum(tol, 1e-300)).max()))
            keep = np.ones(C0.shape, dtype=bool)
            keep[:M, :N] = False
            assert np.array_equal(_bits(got)[keep], _bits(C0)[keep]), 'the padding of C was written'


def test_gemm_rejects_an_epilogue_on_a_split(cuda_device, hip_lib):
    import torch
    from learn_region_grow_amd.lrgnet import _ptr, _stream_ptr
    x = torch.ones((64, 64), dtype=torch.float32, device=cuda_device)
    C = torch.full((64, 64), -3.0, dtype=torch.float32, device=cuda_device)
    for add, mask in [(x, None), (None, x), (x, x)]:
        assert hip_lib.lrg_gemm_f32(64, 64, 64, _ptr(x), 64, 0, _ptr(x), 64, 0, _ptr(C), 64, _ptr(add), _ptr(mask), 2, _stream_ptr()) == EINVAL - 2
    torch.cuda.synchronize()
    assert (C == -3.0).all()


# ---------------------------------------------- 6. the trainer against the oracle at the shapes it really runs ----------------------------------------------
def batch(rs, B, Ni, Nn, F):
    """test_gpu_train.batch with the two point counts apart (the same draws in the same order when they are equal)."""
    xi, xn = (rs.randn(B, Ni, F) * 0.5).astype(np.float32), (rs.randn(B, Nn, F) * 0.5).astype(np.float32)
    xi[0, Ni // 2:] = xi[0, rs.randint(0, Ni // 2, Ni - Ni // 2)]      # a padded set: duplicated rows tie in the max-pool
    am, rm = rs.randint(0, 2, (B, Nn)).astype(np.int32), (rs.rand(B, Ni) < 0.2).astype(np.int32)
    return xi, xn, am, rm


# (lite, F, B, Ni, Nn): split = 2 in every dW; split = 2 on the lite-1 path (identity GEMM); Ni != Nn twice; B = 1
TRAINER_SHAPES = [(0, 13, 34, 64, 64), (1, 13, 40, 64, 64), (0, 13, 2, 64, 128), (2, 12, 3, 128, 64), (0, 13, 1, 64, 64)]
# batch seeds for which no row of either head has |l1 - l0| <= 1e-3 max|logit| in the float64 forward (found on the CPU, asserted below)
TRAINER_SEEDS = {(0, 13, 34, 64, 64): 257, (1, 13, 40, 64, 64): 0, (0, 13, 2, 64, 128): 1, (2, 12, 3, 128, 64): 3, (0, 13, 1, 64, 64): 1,
                 (0, 13, 2, 64, 64): 3}                            # the last one: the batches with an empty remove class (remove head only)


@functools.lru_cache(maxsize=None)
def _case(shape, remove=None):
    """Weights, batch and both oracle runs of a shape, computed once; remove = 0 / 1 makes every remove label that value."""
    lite, F, B, Ni, Nn = shape
    w = synthetic.make_synthetic_weights(feature_size=F, lite=lite, **WEIGHT_KW)
    xi, xn, am, rm = batch(np.random.RandomState(TRAINER_SEEDS[shape]), B, Ni, Nn, F)
    if remove is not None:
        rm[:] = remove
    loss, G, sc = train_ref.loss_and_grads(w, xi, xn, am, rm, lite=lite)
    _, G32, _ = train_ref.loss_and_grads(w, xi, xn, am, rm, lite=lite, dtype=np.float32)
    for a in tuple(G.values()) + tuple(G32.values()):
        a.setflags(write=False)
    return dict(w=w, batch=(xi, xn, am, rm), loss=loss, G=G, G32=G32, scalars=sc)


def _trainer(shape, dev):
    from learn_region_grow_amd.train import LrgNetTrainer
    lite, F, B, Ni, Nn = shape
    return LrgNetTrainer(B, Ni, Nn, F, lite, device=dev).load_weights(_case(shape)['w'])


def _check_gradients(tr, case):
    """Per tensor: GPU error <= max(8 x the float32 oracle's error, 2e-5 max|G|), both against the float64 oracle.  The GPU
    differs from the float32 oracle by accumulation order (MFMA tiles, atomics of the split, two-pass column sums)."""
    got = tr.grads_numpy()
    worst = 0.0
    for k in sorted(case['G']):
        G = case['G'][k]
        scale = float(np.abs(G).max())
        err32 = float(np.abs(case['G32'][k] - G).max())
        err = float(np.abs(got[k] - G).max())
        tol = max(8 * err32, 2e-5 * scale)
        worst = max(worst, err / tol)
        print('%-24s max|G| %.3e  gpu err %.3e  f32-oracle err %.3e  gpu/f32 %.2f  gpu/tol %.3f' %
              (k, scale, err, err32, err / max(err32, 1e-300), err / max(tol, 1e-300)))
        assert np.isfinite(got[k]).all(), k
        assert err <= tol, k
    print('worst gpu err / tol %.3f' % worst)


def _rates(logits, labels):
    """tp / (pp + 1), tp / (lp + 1) (learn_region_grow_util.py:176-184) from float64 logits; also the smallest |l1 - l0| relative
    to the largest |logit|."""
    pred, y = logits[..., 1] > logits[..., 0], labels != 0
    tp, pp, lp = float((pred & y).sum()), float(pred.sum()), float(y.sum())
    return tp / (pp + 1), tp / (lp + 1), float(np.abs(logits[..., 1] - logits[..., 0]).min() / np.abs(logits).max())


@pytest.mark.parametrize('shape', TRAINER_SHAPES, ids=lambda s: 'lite%d-F%d-B%d-Ni%d-Nn%d' % s)
def test_trainer_matches_the_oracle(cuda_device, shape):
    """backward(): loss (rtol 2e-5), gradients (_check_gradients), accuracies, precision and recall.  The gradient buffer starts
    as NaN, so every element must be written and a split reduction must zero its slice first.  No float64 logit pair of the batch
    is closer than 1e-3 max|logit| (asserted), so float32 logits cannot flip a prediction and the four ratios are exact.
    evaluate() then returns the same dictionary, every value equal (lrg_ce_grad sums the loss in a fixed order; the counters are
    integers), and touches neither the gradient buffer, the weights nor t."""
    lite, F, B, Ni, Nn = shape
    case = _case(shape)
    xi, xn, am, rm = case['batch']
    tr = _trainer(shape, cuda_device)
    tr.gflat.fill_(float('nan'))
    sc = tr.backward(xi, xn, am, rm)
    np.testing.assert_allclose(sc['loss'], case['loss'], rtol=2e-5)
    np.testing.assert_allclose(sc['add_loss'], case['scalars']['add_loss'], rtol=2e-5)
    np.testing.assert_allclose(sc['remove_loss'], case['scalars']['remove_loss'], rtol=2e-5)
    _check_gradients(tr, case)
    add, rmv = lrgnet_ref.forward(case['w'], xi, xn, lite=lite, dtype=np.float64)
    a_prc, a_rcl, a_margin = _rates(add, am)
    r_prc, r_rcl, r_margin = _rates(rmv, rm)
    print('margins: add %.3e remove %.3e' % (a_margin, r_margin))
    assert min(a_margin, r_margin) > 1e-3
    assert (sc['add_prc'], sc['add_rcl'], sc['remove_prc'], sc['remove_rcl']) == (a_prc, a_rcl, r_prc, r_rcl)
    assert (sc['add_acc'], sc['remove_acc']) == (case['scalars']['add_acc'], case['scalars']['remove_acc'])
    # evaluate(): the validation loop's call
    w_before, t_before = tr.flat.clone(), tr.step
    tr.gflat.fill_(-777.25)
    ev = tr.evaluate(xi, xn, am, rm)
    assert ev == sc
    assert (tr.gflat == -777.25).all() and np.array_equal(_bits(tr.flat.cpu().numpy()), _bits(w_before.cpu().numpy())) and tr.step == t_before


@pytest.mark.parametrize('remove', [0, 1])
def test_trainer_with_an_empty_remove_class(cuda_device, remove):
    """Every remove label 0 / 1: the empty class contributes nothing (w = 0 where the reference has its tf.cond), the losses stay
    finite, the gradients match."""
    shape = (0, 13, 2, 64, 64)
    case = _case(shape, remove)
    tr = _trainer(shape, cuda_device)
    tr.gflat.fill_(float('nan'))
    sc = tr.backward(*case['batch'])
    print('loss %.4f (oracle %.4f)' % (sc['loss'], case['loss']))
    assert all(np.isfinite(v) for v in sc.values())
    np.testing.assert_allclose(sc['loss'], case['loss'], rtol=2e-5)
    np.testing.assert_allclose(sc['remove_loss'], case['scalars']['remove_loss'], rtol=2e-5)
    _check_gradients(tr, case)
    xi, xn, am, rm = case['batch']
    _, rmv = lrgnet_ref.forward(case['w'], xi, xn, lite=shape[0], dtype=np.float64)
    r_prc, r_rcl, r_margin = _rates(rmv, rm)
    assert r_margin > 1e-3                                          # no float64 logit pair close enough for float32 to flip it
    assert (sc['remove_prc'], sc['remove_rcl']) == (r_prc, r_rcl)


@pytest.mark.parametrize('shape', [(0, 13, 34, 64, 64), (2, 12, 3, 128, 64)], ids=lambda s: 'lite%d-F%d-B%d-Ni%d-Nn%d' % s)
def test_train_step_is_adam_on_the_trainers_own_gradients(cuda_device, shape):
    """Three train_step calls: after each, the flat weights, m and v carry the bits of the float32 restatement (adam_f32) applied
    to the trainer's own gradients, so the optimiser is checked without the gradients' error."""
    case = _case(shape)
    tr = _trainer(shape, cuda_device)
    flat = lambda d: np.concatenate([d[k].reshape(-1) for k in tr.names])
    p, m, v = flat(tr.weights_numpy()), np.zeros(tr.flat.numel(), np.float32), np.zeros(tr.flat.numel(), np.float32)
    for t in range(1, 4):
        tr.train_step(*case['batch'])
        assert tr.step == t
        g = flat(tr.grads_numpy())
        p, m, v = adam_f32(p, g, m, v, adam_lr_t(tr.lr, tr.b1, tr.b2, t), tr.b1, tr.b2, tr.eps)
        for name, got, want in (('weights', tr.flat, p), ('m', tr.m, m), ('v', tr.v, v)):
            bad = _bits(got.cpu().numpy()) != _bits(want)
            assert not bad.any(), 't=%d %s: %d of %d differ' % (t, name, bad.sum(), bad.size)
        assert np.array_equal(_bits(flat(tr.weights_numpy())), _bits(p))
