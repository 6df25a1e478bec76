"""GPU: the PointNet2 baseline (learn_region_grow_amd.pointnet2, csrc/lrg_pointnet2.hip, lrg_baseline_segment_labels) against the
NumPy restatement tests/pointnet2_ref.py.

The bound.  On the very inputs of each comparison d = max |forward(float32) - forward(float64)| of the restatement over the
compared tensor and s = max |forward(float64)|; the device must lie within 8 d + 1e-6 s of the float64 values.  Nothing in it
comes from the kernels.  Measured on the CPU from the restatement alone, on the four cells of ``cells_room`` (435 / 465 points, a
single point, exactly 1024):

    weights (13 classes, xyz only, seed 1)         weights (260 classes, colour, seed 2)
    tensor   d          s       bound              d          s       bound
    sa1      2.24e-08   0.178   3.57e-07           1.08e-07   0.432   1.29e-06
    sa2      4.12e-08   0.173   5.02e-07           5.61e-08   0.237   6.86e-07
    sa3      4.97e-08   0.201   5.98e-07           6.95e-08   0.253   8.09e-07
    sa4      8.75e-08   0.214   9.14e-07           1.18e-07   0.231   1.17e-06
    fp1      1.10e-07   0.249   1.13e-06           1.32e-07   0.228   1.29e-06
    fp2      1.60e-07   0.251   1.53e-06           1.77e-07   0.226   1.64e-06
    fp3      1.60e-07   0.232   1.51e-06           1.24e-07   0.193   1.18e-06
    fp4      9.70e-08   0.269   1.04e-06           1.08e-07   0.320   1.19e-06
    logits   1.09e-07   0.271   1.15e-06           9.98e-08   0.225   1.02e-06

Faults planted in the float64 restatement, one at a time, move the logits by (260 classes, colour; in multiples of that bound):
layer1/bias0 dropped 7.96e-03 (7 776 x), the ReLU after layer2/bias1 skipped 6.87e-03 (6 711 x), sample 31's row used twice at
level 3 5.17e-05 (50 x; at level 3 the level's own features move by 9.2e-03, 11 000 x their bound; at levels 1 and 2 of these
cells samples 30 and 31 are the same row already -- the radius holds fewer than 31 distinct rows -- so the fault changes nothing
there, and the kernel tests plant it on rows that are all distinct), the skip features of fa_layer4 shifted by one channel
7.40e-02 (72 346 x).  test_bound_catches_planted_faults asserts these.  Points whose float64 top-two logit gap is within twice the
bound: 0 of 1 925 (13 classes), 2 of 1 925 (260 classes).

On an MI355X the device's distance from the float64 values was 9.5e-08 on the logits (260 classes; 1.1e-07 with 13 classes) and
5.4e-08 .. 1.6e-07 on the levels' features: the restatement's own float32 distance, a ninth of the bound.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import pointnet2_ref as R
from conftest import REPO
from learn_region_grow_amd import pointnet2 as P  # noqa: F401  (the module under test: without it nothing here can run)

pytestmark = pytest.mark.gpu
EINVAL = -1000
I32P = ctypes.POINTER(ctypes.c_int32)


def bound_of(f32, f64):
    d = np.abs(np.asarray(f32, np.float64) - f64).max()
    s = np.abs(f64).max()
    return 8.0 * d + 1e-6 * s, d, s


def check(name, got, f32, f64):
    bound, d, s = bound_of(f32, f64)
    err = np.abs(np.asarray(got, np.float64) - f64).max()
    print('%s: d %.3e s %.3e bound %.3e device error %.3e' % (name, d, s, bound, err))
    assert np.asarray(got).shape == f64.shape
    assert err <= bound, '%s: device error %.3e > bound %.3e (d %.3e, s %.3e)' % (name, err, bound, d, s)


def cells_room(seed):
    """Equalised points (one per 0.1 m voxel, jittered inside it) that fall into four 1 m cells: two of a few hundred points, one
    of a single point and one of exactly 1024."""
    rng = np.random.RandomState(seed)

    def vox(n, x0, x1, y0, y1, z1):
        g = np.stack(np.meshgrid(np.arange(x0, x1), np.arange(y0, y1), np.arange(0, z1), indexing='ij'), -1).reshape(-1, 3)
        g = g[rng.choice(len(g), n, replace=False)]
        return np.concatenate([(g + rng.uniform(-0.45, 0.45, g.shape)) * 0.1, rng.uniform(0, 1, (n, 3))], axis=1)
    parts = [vox(900, -4, 15, -4, 5, 25), np.array([[5.1, 5.2, 0.7, .2, .3, .4]]), vox(1024, 96, 105, 96, 105, 25)]
    p = np.concatenate(parts).astype(np.float32)
    return p[rng.permutation(len(p))]


def dev(a, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def pack(lib, layers, device):
    import torch
    sizes = [lib.lrg_pointnet2_packed_floats(w.shape[0], w.shape[1]) for w, _ in layers]
    assert all(s == ((w.shape[0] + 31) // 32 * 32 + 1) * ((w.shape[1] + 31) // 32 * 32) for s, (w, _) in zip(sizes, layers))
    packed = torch.zeros(sum(sizes), dtype=torch.float32, device=device)
    off = 0
    for (w, b), s in zip(layers, sizes):
        wd, bd = dev(w, device), dev(b, device)
        assert lib.lrg_pointnet2_pack_layer(w.shape[0], w.shape[1], ptr(wd), ptr(bd), ptr(packed[off:]), None) == 0
        off += s
    torch.cuda.synchronize()
    return packed


def run_group(lib, device, xyz, new_xyz, points, idx, layers, packed=None, nsample=32):
    import torch
    b, n, _ = xyz.shape
    m = new_xyz.shape[1]
    c = 0 if points is None else points.shape[2]
    widths = np.array([w.shape[1] for w, _ in layers], np.int32)
    packed = pack(lib, layers, device) if packed is None else packed
    out = torch.full((b, m, int(widths[-1])), np.nan, dtype=torch.float32, device=device)
    t = [dev(xyz, device), dev(new_xyz, device), None if points is None else dev(points, device), dev(idx.astype(np.int32), device)]
    rc = lib.lrg_pointnet2_group_mlp(b, n, m, nsample, c, ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(t[3]), widths.ctypes.data_as(I32P), ptr(packed),
                                     ptr(out), None)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def run_rows(lib, device, a, b, layers, relu_last, packed=None):
    import torch
    r = a.shape[0]
    widths = np.array([w.shape[1] for w, _ in layers], np.int32)
    packed = pack(lib, layers, device) if packed is None else packed
    out = torch.full((r, int(widths[-1])), np.nan, dtype=torch.float32, device=device)
    ta, tb = dev(a, device), None if b is None else dev(b, device)
    rc = lib.lrg_pointnet2_row_mlp(r, a.shape[1], 0 if b is None else b.shape[1], ptr(ta), ptr(tb), len(layers), widths.ctypes.data_as(I32P),
                                   1 if relu_last else 0, ptr(packed), ptr(out), None)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


# ---- the kernels alone, through the C-ABI -------------------------------------------------------------------------------------
@pytest.mark.parametrize('widths', [(32, 32, 64), (256, 256, 512)])
@pytest.mark.parametrize('cin', [3, 6, 67, 131, 259])
def test_group_mlp(hip_lib, cuda_device, cin, widths):
    rng = np.random.RandomState(cin + widths[0])
    layers = R.random_layers(rng, (cin,) + widths)
    packed = pack(hip_lib, layers, cuda_device)
    n = 40
    for b, m in ((1, 1), (1, 2), (1, 31), (1, 33), (3, 5)):
        xyz = rng.uniform(0, 1, (b, n, 3)).astype(np.float32)
        new_xyz = rng.uniform(0, 1, (b, m, 3)).astype(np.float32)
        points = rng.uniform(-1, 1, (b, n, cin - 3)).astype(np.float32) if cin > 3 else None       # cin == 3: points = NULL
        idx = np.stack([np.stack([rng.permutation(n)[:32] for _ in range(m)]) for _ in range(b)]).astype(np.int32)
        idx[:, 0, 5:] = idx[:, 0, :1]                                # the ball query's padding: the first hit repeated
        if m > 1:
            idx[:, 1, :] = idx[:, 1, :1]                             # a group of one point
        rc, got = run_group(hip_lib, cuda_device, xyz, new_xyz, points, idx, layers, packed)
        assert rc == 0
        f64 = R.group_mlp(xyz, new_xyz, points, idx, layers, np.float64)
        f32 = R.group_mlp(xyz, new_xyz, points, idx, layers, np.float32)
        check('group_mlp cin %d widths %s b %d m %d' % (cin, widths, b, m), got, f32, f64)
        if (b, m) == (1, 33):                                        # the bound sees sample 31's row used in place of sample 30
            dup = idx.copy()
            dup[:, :, 30] = dup[:, :, 31]
            assert np.abs(R.group_mlp(xyz, new_xyz, points, dup, layers, np.float64) - f64).max() > bound_of(f32, f64)[0]


@pytest.mark.parametrize('n_layers', [1, 2, 3])
@pytest.mark.parametrize('ca,cb', [(512, 256), (128, 0), (128, 3)])
def test_row_mlp(hip_lib, cuda_device, ca, cb, n_layers):
    rng = np.random.RandomState(ca + cb + n_layers)
    a_all = rng.uniform(-1, 1, (1025, ca)).astype(np.float32)
    b_all = rng.uniform(-1, 1, (1025, cb)).astype(np.float32) if cb else None
    for last in (13, 40, 260):
        layers = R.random_layers(rng, (ca + cb,) + (256, 128)[:n_layers - 1] + (last,))
        packed = pack(hip_lib, layers, cuda_device)
        ref = {relu: (R.row_mlp(a_all, b_all, layers, relu, np.float32), R.row_mlp(a_all, b_all, layers, relu, np.float64)) for relu in (True, False)}
        assert (ref[False][1] < 0).any()                             # the flag matters on these inputs
        for r in (1, 31, 32, 33, 1025):
            for relu in (True, False):
                rc, got = run_rows(hip_lib, cuda_device, a_all[:r], None if b_all is None else b_all[:r], layers, relu, packed)
                assert rc == 0
                # a row's value does not depend on r: the reference of the first r rows is the first r rows of the reference
                check('row_mlp (%d, %d) layers %d last %d r %d relu %d' % (ca, cb, n_layers, last, r, relu), got, ref[relu][0][:r], ref[relu][1][:r])


def test_mlp_argument_errors(hip_lib, cuda_device):
    import torch
    rng = np.random.RandomState(0)
    layers = R.random_layers(rng, (6, 32, 32, 64))
    xyz = rng.uniform(0, 1, (1, 40, 3)).astype(np.float32)
    pts = rng.uniform(0, 1, (1, 40, 3)).astype(np.float32)
    idx = rng.randint(0, 40, (1, 2, 32))
    assert run_group(hip_lib, cuda_device, xyz, xyz[:, :2], pts, idx, layers)[0] == 0
    for ns in (16, 31, 33, 64):
        assert EINVAL - 100 < run_group(hip_lib, cuda_device, xyz, xyz[:, :2], pts, idx, layers, nsample=ns)[0] <= EINVAL
    t = [dev(xyz, cuda_device), dev(pts, cuda_device), dev(idx.astype(np.int32), cuda_device), pack(hip_lib, layers, cuda_device),
         torch.zeros((2, 64), dtype=torch.float32, device=cuda_device)]

    def group(widths, c=3, args=None, b=1, n=40, m=2):
        a = [ptr(t[0]), ptr(t[0]), ptr(t[1]), ptr(t[2]), None if widths is None else np.array(widths, np.int32).ctypes.data_as(I32P), ptr(t[3]), ptr(t[4])]
        for k in (args or ()):
            a[k] = None
        return hip_lib.lrg_pointnet2_group_mlp(b, n, m, 32, c, a[0], a[1], a[2], a[3], a[4], a[5], a[6], None)
    assert group((32, 32, 64)) == 0
    for bad in ((33, 32, 64), (32, 48, 64), (32, 32, 65), (32, 32, 0), (544, 32, 64), (32, 32, 1024)):       # not a multiple of 32, above the cap
        assert EINVAL - 100 < group(bad) <= EINVAL, bad
    for k in range(7):                                               # NULL where a pointer is read
        assert EINVAL - 100 < group((32, 32, 64), args=(k,)) <= EINVAL, k
    assert EINVAL - 100 < group((32, 32, 64), c=1022) <= EINVAL and EINVAL - 100 < group((32, 32, 64), c=-1) <= EINVAL
    assert EINVAL - 100 < group((32, 32, 64), n=0) <= EINVAL and EINVAL - 100 < group((32, 32, 64), b=-1) <= EINVAL
    assert group((32, 32, 64), c=0, args=(2,)) == 0                 # points may be NULL with c == 0 (then the level's kernel0 has 3 rows)

    rl = R.random_layers(rng, (9, 64, 32, 13))
    tr = [dev(rng.uniform(0, 1, (5, 6)).astype(np.float32), cuda_device), dev(rng.uniform(0, 1, (5, 3)).astype(np.float32), cuda_device),
          pack(hip_lib, rl, cuda_device), torch.zeros((5, 64), dtype=torch.float32, device=cuda_device)]

    def rows(widths, r=5, ca=6, cb=3, relu=1, args=None, n_layers=None):
        a = [ptr(tr[0]), ptr(tr[1]), None if widths is None else np.array(widths, np.int32).ctypes.data_as(I32P), ptr(tr[2]), ptr(tr[3])]
        for k in (args or ()):
            a[k] = None
        return hip_lib.lrg_pointnet2_row_mlp(r, ca, cb, a[0], a[1], len(widths) if n_layers is None else n_layers, a[2], relu, a[3], a[4], None)
    assert rows((64, 32, 13)) == 0 and rows((64, 32, 13), r=0) == 0
    for bad in ((63, 32, 13), (64, 40, 13), (64, 32, 513), (64, 32, 0), (544, 32, 13)):
        assert EINVAL - 100 < rows(bad) <= EINVAL, bad
    for k in range(5):
        assert EINVAL - 100 < rows((64, 32, 13), args=(k,)) <= EINVAL, k
    assert EINVAL - 100 < rows((64, 32, 13), n_layers=0) <= EINVAL and EINVAL - 100 < rows((64, 32, 13, 13), n_layers=4) <= EINVAL
    assert EINVAL - 100 < rows((64, 32, 13), r=-1) <= EINVAL and EINVAL - 100 < rows((64, 32, 13), relu=2) <= EINVAL
    assert EINVAL - 100 < rows((64, 32, 13), ca=0) <= EINVAL and EINVAL - 100 < rows((64, 32, 13), ca=1000, cb=25) <= EINVAL
    assert EINVAL - 100 < rows((64, 32, 13), cb=-1) <= EINVAL
    assert hip_lib.lrg_pointnet2_packed_floats(0, 32) == 0 and hip_lib.lrg_pointnet2_packed_floats(1025, 32) == 0
    assert hip_lib.lrg_pointnet2_packed_floats(3, 513) == 0 and hip_lib.lrg_pointnet2_packed_floats(3, 32) == 33 * 32
    assert EINVAL - 100 < hip_lib.lrg_pointnet2_pack_layer(3, 32, None, ptr(tr[1]), ptr(tr[3]), None) <= EINVAL
    assert EINVAL - 100 < hip_lib.lrg_pointnet2_pack_layer(3, 600, ptr(tr[0]), ptr(tr[1]), ptr(tr[3]), None) <= EINVAL
    torch.cuda.synchronize()


# ---- the network ----------------------------------------------------------------------------------------------------------------
CONFIGS = {'s3dis-xyz': (13, False, 1), 'kitti-rgb': (260, True, 2)}
_CASES = {}


def case(name, device):
    """The cells, weights, restatement (float64 and float32) and device network of a configuration, computed once."""
    if name not in _CASES:
        from learn_region_grow_amd import pointnet2 as P
        nc, rgb, seed = CONFIGS[name]
        room = cells_room(seed)
        batch, members, keys = P.cell_inputs(room, 1.0)
        assert len(members) == 4 and {1, 1024} <= set(len(m) for m in members)
        w = R.random_weights(seed, nc, rgb)
        l64, lv64 = R.forward(batch, w, np.float64)
        l32, lv32 = R.forward(batch, w, np.float32)
        _CASES[name] = dict(room=room, batch=batch, members=members, weights=w, l64=l64, lv64=lv64, l32=l32, lv32=lv32,
                            net=P.PointNet2HIP(w, device=device), bound=bound_of(l32, l64)[0])
    return _CASES[name]


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_network_levels_and_logits(cuda_device, name):
    c = case(name, cuda_device)
    assert (c['net'].num_class, c['net'].rgb_features) == CONFIGS[name][:2]
    got, lv = c['net'].logits(c['batch'], return_levels=True)
    for k in range(4):                                               # xyz only: the ops are bit for bit
        for key in ('fps', 'new_xyz', 'idx'):
            assert np.array_equal(lv['sa'][k][key], c['lv64']['sa'][k][key]), (k, key)
        assert np.array_equal(lv['fp'][k]['nn_idx'], c['lv64']['fp'][k]['nn_idx']), k
    for k in range(4):
        check('%s sa%d' % (name, k + 1), lv['sa'][k]['features'], c['lv32']['sa'][k]['features'], c['lv64']['sa'][k]['features'])
    for k in range(4):
        check('%s fp%d' % (name, k + 1), lv['fp'][k]['features'], c['lv32']['fp'][k]['features'], c['lv64']['fp'][k]['features'])
    check('%s logits' % name, got, c['l32'], c['l64'])
    assert got.dtype == np.float32 and got.shape == (4, 1024, CONFIGS[name][0])
    assert np.array_equal(got, c['net'].logits(c['batch']))         # without return_levels: the same bits


def test_bound_catches_planted_faults(cuda_device):
    c = case('kitti-rgb', cuda_device)
    for m in ({'drop_bias': 'layer1/bias0'}, {'skip_relu': 'layer2/bias1'}, {'dup_sample': 3}, {'shift_skip': 4}):
        lm, _ = R.forward(c['batch'], c['weights'], np.float64, mutate=m)
        dist = np.abs(lm - c['l64']).max()
        print('%s: logits move by %.3e = %.0f x the bound %.3e' % (m, dist, dist / c['bound'], c['bound']))
        assert dist > c['bound'], m


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_classes(cuda_device, name):
    c = case(name, cuda_device)
    got = c['net'].classify([c['room']], area='5')[0]
    assert got.dtype == np.int32 and got.shape == (len(c['room']),)
    want = np.zeros(len(c['room']), np.int64)
    gap = np.zeros(len(c['room']))
    for k, idx in enumerate(c['members']):
        lg = c['l64'][k, :len(idx)]
        want[idx] = lg.argmax(axis=1)
        top = np.sort(lg, axis=1)
        gap[idx] = top[:, -1] - top[:, -2]
    clear = gap > 2 * c['bound']
    print('%s: %d of %d points within twice the bound %.3e of a tie' % (name, (~clear).sum(), len(clear), c['bound']))
    assert (~clear).mean() <= 0.05
    assert np.array_equal(got[clear], want[clear])
    assert np.array_equal(c['net'].classify([dict(points=c['room'])], area='scannet')[0], got)        # a dict with 'points' is a room too


def test_independence_of_batch_and_chunk(cuda_device):
    from learn_region_grow_amd import pointnet2 as P
    c = case('s3dis-xyz', cuda_device)
    net, batch = c['net'], c['batch']
    alone = [net.logits(batch[k:k + 1])[0] for k in range(4)]
    five = net.logits(np.concatenate([batch, batch[:1]]))
    many = net.logits(batch[np.arange(P.CHUNK_CELLS + 3) % 4])      # crosses the chunk
    for k in range(4):
        assert np.array_equal(five[k], alone[k]), k
    assert np.array_equal(five[4], alone[0])
    for k in range(P.CHUNK_CELLS + 3):
        assert np.array_equal(many[k], alone[k % 4]), k
    assert np.array_equal(net.logits(batch), net.logits(batch))     # two calls, the same bits


# ---- segmentation -------------------------------------------------------------------------------------------------------------
def class_room(seed, shift=0):
    """Nine rows of 33 voxels, 0.2 m apart, whose classes form runs along x with known sizes (10 and 11 among them), classes above 64
    among them, in shuffled point order."""
    rng = np.random.RandomState(seed)
    pts, cls = [], []
    for y in range(9):
        runs = [(70, 10), (300, 11), (5, 12)] if y % 3 == 0 else ([(1000 + y, 33)] if y % 3 == 1 else [(y, 3), (259, 30)])
        x = 0
        for cl, n in runs:
            for _ in range(n):
                pts.append([x * 0.1, y * 0.2 + shift, 0.0])         # rows 0.2 m apart: only the runs along x touch
                cls.append(cl)
                x += 1
    pts = np.concatenate([np.array(pts), rng.uniform(0, 1, (len(pts), 3))], axis=1).astype(np.float32)
    order = rng.permutation(len(pts))
    return pts[order], np.array(cls, np.int32)[order]


def test_segment_known_structure_and_batching(cuda_device):
    from learn_region_grow_amd import pointnet2 as P
    big = cells_room(3)
    rooms = [class_room(1), class_room(2, shift=50.0), (big, (np.round(big[:, 2] / 0.5).astype(np.int32) * 37) % 301)]   # layers of classes up to 300
    dicts = [dict(points=p) for p, _ in rooms]
    want = [R.segment(p, c) for p, c in rooms]
    got = P.segment(dicts, [c for _, c in rooms], device=cuda_device)
    for k in range(3):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), k
    for k in range(2):
        p, c = rooms[k]
        sizes = np.bincount(want[k])
        assert set(sizes[1:].tolist()) == {11, 12, 33, 30} and sizes[0] == 3 * 10 + 3 * 3
        assert (want[k][c == 70] == 0).all() and (want[k][c == 300] > 0).all()            # 10 points: no cluster; 11: a cluster
    for k in range(3):                                               # a room alone gives the same labels
        assert np.array_equal(P.segment(dicts[k:k + 1], [rooms[k][1]], device=cuda_device)[0], got[k])
    out, cnt = P.segment(dicts, [c for _, c in rooms], device=cuda_device, return_counts=True)
    assert [int(x) for x in cnt] == [int(w.max()) for w in want]


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def test_end_to_end_and_cli(tmp_path, cuda_device):
    from learn_region_grow_amd import checkpoint, io, metrics, synthetic
    from learn_region_grow_amd import pointnet2 as P
    raw = [synthetic.area5_shaped_room(2500, 11).astype(np.float32), synthetic.area5_shaped_room(1800, 12).astype(np.float32)]
    w = R.random_weights(5, 13, True)
    net = P.PointNet2HIP(w, device=cuda_device)
    rooms = [P.prepare_room(r, device=cuda_device) for r in raw]
    for r, x in zip(rooms, raw):
        p, eq, uq = R.equalize(x[:, :6])
        assert np.array_equal(r['points'], p) and np.array_equal(r['equalized_idx'], eq) and np.array_equal(r['unequalized_idx'], uq)
    classes = net.classify(rooms, area='5')
    labels = P.segment(rooms, classes, device=cuda_device)
    lines = []
    for k, r in enumerate(rooms):
        assert np.array_equal(labels[k], R.segment(r['points'], classes[k])), k            # the restatement's labels, given the device's classes
        lines.append(metrics.room_line('5', k, metrics.room_metrics(raw[k][r['equalized_idx'], 6].astype(int), labels[k].astype(np.int64))))
    h5 = str(tmp_path / 'rooms.h5')
    io.saveToH5(h5, raw)
    ck = str(tmp_path / 'm' / 'pn2.ckpt')
    checkpoint.write_bundle(ck, w)
    outs = {}
    for how in ('host', 'device'):
        p = subprocess.run([sys.executable, os.path.join(REPO, 'pointnet2.py'), '--h5', h5, '--area', '5', '--ckpt', ck, '--metrics', how,
                            '--save', str(tmp_path / how)], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        outs[how] = [l for l in p.stdout.rstrip('\n').split('\n') if not l.startswith('Saved to ')]      # io.savePLY names each file it writes
    out = outs['host']
    assert out[0] == 'Restored from %s' % ck
    assert [l for l in out if l.startswith('Area ')] == lines
    import re
    for k in range(2):                                               # benchmarks.py's timing line, then the room's metric line
        assert re.fullmatch(r' %d points: \d+\.\d\ds' % len(raw[k]), out[1 + 2 * k]), out[1 + 2 * k]
        assert re.fullmatch(r'Area 5 room %d NMI: \d\.\d\d AMI: -?\d\.\d\d ARS: -?\d\.\d\d PRC: \d\.\d\d RCL: \d\.\d\d IOU: \d\.\d\d' % k, out[2 + 2 * k])
    assert re.fullmatch(r'NMI: \d\.\d\d\+-\d\.\d\d AMI: .* IOU \d\.\d\d\+-\d\.\d\d', out[-1]) and len(out) == 6
    strip = lambda ls: [l for l in ls if ' points: ' not in l]      # the timing lines differ from run to run
    assert strip(outs['device']) == strip(out)
    for k in range(2):
        ply = (tmp_path / 'host' / ('%d.ply' % k)).read_text()
        assert ply.startswith('ply\nformat ascii 1.0\nelement vertex %d\n' % len(raw[k]))
        assert ply == (tmp_path / 'device' / ('%d.ply' % k)).read_text()
