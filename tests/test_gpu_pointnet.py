"""GPU: the plain PointNet baseline (learn_region_grow_amd.pointnet, csrc/lrg_pointnet.hip, lrg_baseline_segment_labels) against the
NumPy restatement tests/pointnet_ref.py.

The bound, that of tests/test_gpu_pointnet2.py with the same reasoning.  On the very inputs of each comparison
d = max |restatement(float32) - restatement(float64)| over the compared tensor and s = max |restatement(float64)|; the device must
lie within 8 d + 1e-6 s of the float64 values.  Nothing in it comes from the kernels.  Measured on the CPU from the restatement
alone, on the four cells of ``test_gpu_pointnet2.cells_room`` (435 / 465 or 470 / 430 points, a single point, exactly 1024):

    shipped network [64,64,128,512] / [512], 13 classes, seed 1      today's [64,64,64,128,1024] / [512,256], 260 classes, seed 2
    tensor   d          s       bound                                d          s       bound
    skip     1.38e-07   0.405   1.51e-06                             1.20e-07   0.533   1.49e-06
    last     8.82e-08   0.362   1.07e-06                             9.63e-08   0.336   1.11e-06
    pooled   8.46e-08   0.362   1.04e-06                             4.86e-08   0.336   7.25e-07
    logits   1.09e-06   2.534   1.13e-05                             3.07e-06   5.836   3.04e-05

Faults planted in the float64 restatement, one at a time, move the logits by (today's network, 260 classes; in multiples of that
bound): the skip taken from conv[0] 1.07 (35 096 x), the pooled row not subtracted 3.18 (104 784 x), the batch-norm tables of the row
position before 6.82 (224 389 x), the ReLU after the last hidden fc layer skipped 6.16 (202 834 x), the maximum over the first 992
rows only 8.80e-04 (29 x; 55 x with the shipped network).
The last needs a column whose maximum lies in the last 32 rows; only the cell of 1024 points can have one (the padding rows of the
others repeat row 0), and test_bound_catches_planted_faults asserts that it has.  Points whose float64 top-two logit gap is within
twice the bound: 0 of 1 925 with either network.

On an MI355X the device's distance from the float64 values was 3.3e-06 on the logits (today's network, 260 classes; 1.7e-06 with the
shipped one and 13 classes), 5.2e-08 .. 1.4e-07 on skip, last and pooled, and over all comparisons of this file 0.8 .. 2.4 d: the
restatement's own float32 distance, at most 0.22 of the bound.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import pointnet2_ref
import pointnet_ref as R
from conftest import REPO
from learn_region_grow_amd import pointnet as P  # noqa: F401  (the module under test: without it nothing here can run)
from test_gpu_pointnet2 import cells_room

pytestmark = pytest.mark.gpu
EINVAL = -1000
I32P = ctypes.POINTER(ctypes.c_int32)
FAULTS = ('skip_conv0', 'no_subtract', 'bn_shift_rows', 'skip_last_relu', 'pool_992')


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


def dev(a, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def conv_layers(w):
    n = len(R.widths_of(w)[0])
    return [(w['kernel%d' % i].reshape(-1, w['kernel%d' % i].shape[-1]), w['bias%d' % i]) for i in range(n)]


def fc_layers(w):
    n = len(R.widths_of(w)[1]) + 1
    return [(w['fc_weights%d' % j][0], w['fc_bias%d' % j]) for j in range(n)]


def pack(lib, layers, device):
    import torch
    sizes = [lib.lrg_pointnet_packed_floats(w.shape[0], w.shape[1]) for w, _ in layers]
    assert all(s == ((w.shape[0] + 31) // 32 * 32 + 1) * ((w.shape[1] + 31) // 32 * 32) for s, (w, _) in zip(sizes, layers))
    packed = torch.zeros(sum(sizes), dtype=torch.float32, device=device)
    off = 0
    for (w, b), s in zip(layers, sizes):
        wd, bd = dev(w, device), dev(b, device)
        assert lib.lrg_pointnet_pack_layer(w.shape[0], w.shape[1], ptr(wd), ptr(bd), ptr(packed[off:]), None) == 0
        off += s
    torch.cuda.synchronize()
    return packed


def bn_tables(w, device):
    tables = []
    for j in range(len(R.widths_of(w)[1])):
        tables.extend(P.fold_batch_norm(*(w[n] for n in R.bn_names(j))))
    return dev(np.concatenate([t.reshape(-1) for t in tables]), device)


def run_features(lib, device, x, layers, packed, want_last=True):
    import torch
    b = x.shape[0]
    widths = np.array([w.shape[1] for w, _ in layers], np.int32)
    skip = torch.full((b, 1024, int(widths[1])), np.nan, dtype=torch.float32, device=device)
    last = torch.full((b, 1024, int(widths[-1])), np.nan, dtype=torch.float32, device=device) if want_last else None
    pooled = torch.full((b, int(widths[-1])), np.nan, dtype=torch.float32, device=device)
    xd = dev(x, device)
    rc = lib.lrg_pointnet_features(b, len(layers), widths.ctypes.data_as(I32P), ptr(xd), ptr(packed), ptr(skip), ptr(last), ptr(pooled), None)
    torch.cuda.synchronize()
    return rc, skip.cpu().numpy(), None if last is None else last.cpu().numpy(), pooled.cpu().numpy()


def run_head(lib, device, last, skip, pooled, layers, packed, bn):
    import torch
    b = last.shape[0]
    widths = np.array([w.shape[1] for w, _ in layers], np.int32)
    out = torch.full((b, 1024, int(widths[-1])), np.nan, dtype=torch.float32, device=device)
    t = [dev(last, device), dev(skip, device), dev(pooled, device)]
    rc = lib.lrg_pointnet_head(b, last.shape[2], skip.shape[2], ptr(t[0]), ptr(t[1]), ptr(t[2]), len(layers), widths.ctypes.data_as(I32P),
                               ptr(packed), ptr(bn), ptr(out), None)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def kernel_cells(seed):
    """Three cells of network inputs: random rows, a cell of 300 points (the padding repeats row 0) and a cell whose last row is far
    from the others, so that columns have their maximum in the last tile."""
    rng = np.random.RandomState(seed)
    x = rng.uniform(-0.5, 0.5, (3, 1024, 6)).astype(np.float32)
    x[:, :, 2:] = rng.uniform(0, 1, (3, 1024, 4))
    x[1, 300:] = x[1, 0]
    x[2, 1023] = [0.9, -0.9, 2.5, 1.0, 0.0, 1.0]
    return x


# ---- the kernels alone, through the C-ABI -------------------------------------------------------------------------------------
WIDTHS = {'shipped': R.SHIPPED, 'current': R.CURRENT,
          'wide-hidden': ((64, 1024, 96), (64,)),                    # a hidden convolution of more than 512 columns: eight tiles per wavefront
          'two-convs': ((96, 32), (32,))}                             # conv[1] is the last layer


@pytest.mark.parametrize('name', sorted(WIDTHS))
def test_features(hip_lib, cuda_device, name):
    conv, fc = WIDTHS[name]
    w = R.random_weights(11, conv, fc, 13)
    x = kernel_cells(12)
    c64, c32 = R.features(x, w, np.float64), R.features(x, w, np.float32)
    assert (c64[-1][2].argmax(axis=0) == 1023).any() and (c64[-1] == 0).any()       # a maximum in the last row; the ReLU cuts
    layers = conv_layers(w)
    packed = pack(hip_lib, layers, cuda_device)
    for b in (1, 2, 3):
        rc, skip, last, pooled = run_features(hip_lib, cuda_device, x[:b], layers, packed)
        assert rc == 0
        # a cell's values do not depend on b: the reference of the first b cells is the first b cells of the reference
        check('%s features b %d skip' % (name, b), skip, c32[1][:b], c64[1][:b])
        check('%s features b %d last' % (name, b), last, c32[-1][:b], c64[-1][:b])
        check('%s features b %d pooled' % (name, b), pooled, c32[-1][:b].max(axis=1), c64[-1][:b].max(axis=1))
        assert np.array_equal(pooled, last.max(axis=1))              # the maximum of the device's own rows, bit for bit
        rc, skip2, none, pooled2 = run_features(hip_lib, cuda_device, x[:b], layers, packed, want_last=False)
        assert rc == 0 and none is None and np.array_equal(skip2, skip) and np.array_equal(pooled2, pooled)


@pytest.mark.parametrize('name,classes', [('shipped', (13, 40, 260, 520)), ('current', (13, 40, 260))])
def test_head(hip_lib, cuda_device, name, classes):
    conv, fc = WIDTHS[name]
    x = kernel_cells(13)
    feat = R.features(x, R.random_weights(14, conv, fc, 13), np.float32)
    last, skip = feat[-1], feat[1]
    pooled = last.max(axis=1)
    for nc in classes:
        w = R.random_weights(15 + nc, conv, fc, nc)
        l64, fc64 = R.head(last, skip, pooled, w, np.float64)
        l32, _ = R.head(last, skip, pooled, w, np.float32)
        assert all((h == 0).any() for h in fc64)                     # the ReLUs cut
        layers = fc_layers(w)
        packed, bn = pack(hip_lib, layers, cuda_device), bn_tables(w, cuda_device)
        for b in (1, 2, 3):
            rc, got = run_head(hip_lib, cuda_device, last[:b], skip[:b], pooled[:b], layers, packed, bn)
            assert rc == 0
            check('%s head classes %d b %d' % (name, nc, b), got, l32[:b], l64[:b])
        if nc == 13:                                                 # the bound sees the tables of the row position before
            moved = np.abs(R.head(last, skip, pooled, w, np.float64, mutate='bn_shift_rows')[0] - l64).max()
            assert moved > bound_of(l32, l64)[0]


def test_argument_errors(hip_lib, cuda_device):
    import torch
    conv, fc = R.SHIPPED
    w = R.random_weights(0, conv, fc, 13)
    cl, fl = conv_layers(w), fc_layers(w)
    t = dict(x=dev(kernel_cells(1)[:1], cuda_device), cp=pack(hip_lib, cl, cuda_device), fp=pack(hip_lib, fl, cuda_device), bn=bn_tables(w, cuda_device),
             skip=torch.zeros((1, 1024, 64), dtype=torch.float32, device=cuda_device), last=torch.zeros((1, 1024, 512), dtype=torch.float32, device=cuda_device),
             pooled=torch.zeros((1, 512), dtype=torch.float32, device=cuda_device), out=torch.zeros((1, 1024, 13), dtype=torch.float32, device=cuda_device))
    bad = lambda rc: EINVAL - 100 < rc <= EINVAL

    def features(widths=conv, cells=1, null=(), n_conv=None):
        a = {k: (None if k in null else ptr(t[k])) for k in ('x', 'cp', 'skip', 'last', 'pooled')}
        wp = None if widths is None else np.array(widths, np.int32).ctypes.data_as(I32P)
        return hip_lib.lrg_pointnet_features(cells, len(widths) if n_conv is None else n_conv, wp, a['x'], a['cp'], a['skip'], a['last'], a['pooled'], None)
    assert features() == 0 and features(null=('last',)) == 0
    for k in ('x', 'cp', 'skip', 'pooled'):
        assert bad(features(null=(k,))), k
    assert bad(features(widths=None, n_conv=4))
    for ws in ((64, 64, 128, 500), (64, 48, 128, 512), (64, 64, 128, 1056), (0, 64, 128, 512), (64,), (64, 64, 64, 64, 64, 64)):
        assert bad(features(widths=ws)), ws
    assert bad(features(cells=-1)) and features(cells=0) == 0 and features(cells=0, null=('x', 'cp', 'skip', 'last', 'pooled')) == 0
    assert bad(features(cells=0, widths=(64, 48, 128, 512)))         # the widths are checked before the count

    def head(widths=(512, 13), cells=1, null=(), c_last=512, c_skip=64, n_fc=None):
        a = {k: (None if k in null else ptr(t[k])) for k in ('last', 'skip', 'pooled', 'fp', 'bn', 'out')}
        wp = None if widths is None else np.array(widths, np.int32).ctypes.data_as(I32P)
        return hip_lib.lrg_pointnet_head(cells, c_last, c_skip, a['last'], a['skip'], a['pooled'], len(widths) if n_fc is None else n_fc, wp,
                                         a['fp'], a['bn'], a['out'], None)
    assert head() == 0
    for k in ('last', 'skip', 'pooled', 'fp', 'bn', 'out'):
        assert bad(head(null=(k,))), k
    assert bad(head(widths=None, n_fc=2))
    for ws in ((500, 13), (544, 13), (512, 0), (512, 1025), (13,), (512, 256, 128, 13), (512, 250, 13)):
        assert bad(head(widths=ws)), ws
    for cl_, cs_ in ((500, 64), (512, 48), (0, 64), (512, 0), (1056, 64), (1024, 1024)):
        assert bad(head(c_last=cl_, c_skip=cs_)), (cl_, cs_)
    assert bad(head(cells=-1)) and head(cells=0) == 0 and head(cells=0, null=('last', 'skip', 'pooled', 'fp', 'bn', 'out')) == 0
    # the caps of the packed image are this network's, and lrg_pointnet2's have not moved
    assert hip_lib.lrg_pointnet_packed_floats(2048, 1024) == 2049 * 1024 and hip_lib.lrg_pointnet_packed_floats(6, 64) == 33 * 64
    assert hip_lib.lrg_pointnet_packed_floats(2049, 32) == 0 and hip_lib.lrg_pointnet_packed_floats(32, 1025) == 0
    assert hip_lib.lrg_pointnet_packed_floats(0, 32) == 0 and hip_lib.lrg_pointnet_packed_floats(32, 0) == 0
    assert hip_lib.lrg_pointnet2_packed_floats(1025, 32) == 0 and hip_lib.lrg_pointnet2_packed_floats(3, 513) == 0
    assert bad(hip_lib.lrg_pointnet_pack_layer(6, 64, None, ptr(t['bn']), ptr(t['out']), None))
    assert bad(hip_lib.lrg_pointnet_pack_layer(6, 64, ptr(t['x']), None, ptr(t['out']), None))
    assert bad(hip_lib.lrg_pointnet_pack_layer(6, 64, ptr(t['x']), ptr(t['bn']), None, None))
    assert bad(hip_lib.lrg_pointnet_pack_layer(6, 1056, ptr(t['x']), ptr(t['bn']), ptr(t['out']), None))
    torch.cuda.synchronize()


# ---- the network ----------------------------------------------------------------------------------------------------------------
CONFIGS = {'shipped-13': (R.SHIPPED, 13, 1), 'current-260': (R.CURRENT, 260, 2)}
_CASES = {}


def case(name, device):
    """The cells, weights, restatement (float64 and float32) and device network of a configuration, computed once."""
    if name not in _CASES:
        (conv, fc), nc, seed = CONFIGS[name]
        room = cells_room(seed)
        batch, members, keys = P.cell_inputs(room, 1.0)
        assert len(members) == 4 and {1, 1024} <= set(len(m) for m in members)
        w = R.random_weights(seed, conv, fc, nc)
        l64, p64 = R.forward(batch, w, np.float64)
        l32, p32 = R.forward(batch, w, np.float32)
        _CASES[name] = dict(room=room, batch=batch, members=members, weights=w, l64=l64, p64=p64, l32=l32, p32=p32,
                            net=P.PointNetHIP(w, device=device), bound=bound_of(l32, l64)[0])
    return _CASES[name]


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_network_parts_and_logits(cuda_device, name):
    c = case(name, cuda_device)
    (conv, fc), nc, _ = CONFIGS[name]
    assert (c['net'].conv_widths, c['net'].fc_widths, c['net'].num_class) == (conv, fc, nc)
    got, parts = c['net'].logits(c['batch'], return_parts=True)
    check('%s skip' % name, parts['skip'], c['p32']['skip'], c['p64']['skip'])
    check('%s last' % name, parts['last'], c['p32']['conv'][-1], c['p64']['conv'][-1])
    check('%s pooled' % name, parts['pooled'], c['p32']['pooled'], c['p64']['pooled'])
    check('%s logits' % name, got, c['l32'], c['l64'])
    assert got.dtype == np.float32 and got.shape == (4, 1024, nc)
    assert np.array_equal(got, c['net'].logits(c['batch']))         # without return_parts: the same bits


def test_bound_catches_planted_faults(cuda_device):
    c = case('current-260', cuda_device)
    full = [k for k, m in enumerate(c['members']) if len(m) == 1024]
    assert len(full) == 1 and (c['p64']['conv'][-1][full[0]].argmax(axis=0) >= 992).any()      # a column maximum in the last 32 rows
    for m in FAULTS:
        lm, _ = R.forward(c['batch'], c['weights'], np.float64, mutate=m)
        dist = np.abs(lm - c['l64']).max()
        print('%s: logits move by %.3e = %.0f x the bound %.3e' % (m, dist, dist / c['bound'], c['bound']))
        assert dist > c['bound'], m


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_classes(cuda_device, name):
    c = case(name, cuda_device)
    got = c['net'].classify([c['room']], area='5')[0]
    assert got.dtype == np.int32 and got.shape == (len(c['room']),)
    want, gap = R.classify(c['room'], c['weights'], 1.0)
    clear = gap > 2 * c['bound']
    print('%s: %d of %d points within twice the bound %.3e of a tie' % (name, (~clear).sum(), len(clear), c['bound']))
    assert (~clear).mean() <= 0.05
    assert np.array_equal(got[clear], want[clear])
    assert np.array_equal(c['net'].classify([dict(points=c['room'])], area='scannet')[0], got)        # a dict with 'points' is a room too


def test_independence_of_batch_and_chunk(cuda_device):
    c = case('shipped-13', cuda_device)
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
    assert net.logits(batch[:0]).shape == (0, 1024, 13)


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def test_end_to_end_and_cli(tmp_path, cuda_device):
    from learn_region_grow_amd import checkpoint, io, metrics, synthetic
    raw = [synthetic.area5_shaped_room(2500, 11).astype(np.float32), synthetic.area5_shaped_room(1800, 12).astype(np.float32)]
    w = R.random_weights(5, *R.CURRENT, 13)
    net = P.PointNetHIP(w, device=cuda_device)
    rooms = [P.prepare_room(r, device=cuda_device) for r in raw]
    classes = net.classify(rooms, area='5')
    labels = P.segment(rooms, classes, device=cuda_device)
    lines = []
    for k, r in enumerate(rooms):
        assert np.array_equal(labels[k], pointnet2_ref.segment(r['points'], classes[k])), k            # the restatement's labels, given the device's classes
        lines.append(metrics.room_line('5', k, metrics.room_metrics(raw[k][r['equalized_idx'], 6].astype(int), labels[k].astype(np.int64))))
    h5 = str(tmp_path / 'rooms.h5')
    io.saveToH5(h5, raw)
    ck = str(tmp_path / 'm' / 'pn.ckpt')
    checkpoint.write_bundle(ck, w)
    outs = {}
    for how in ('host', 'device'):
        p = subprocess.run([sys.executable, os.path.join(REPO, 'pointnet.py'), '--h5', h5, '--area', '5', '--ckpt', ck, '--metrics', how,
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
