"""GPU: the growth trace (lrg_trace_snapshot), the rasteriser (lrg_render_visibility), the shading with its text (lrg_render_shade) and the
animate_region_growing.py driver, all BIT FOR BIT against the NumPy twin of tests/animate_ref.py (pinned by test_animate_host.py).  The
oracle behind the trace is driven by the GPU's own logits, as in test_gpu_grow.py, so that every mask must agree exactly."""
import os
import subprocess
import sys

import numpy as np
import pytest

import animate_ref as ar
import step_audit
from conftest import REPO, seed_without_near_tie
from learn_region_grow_amd import io as lio
from learn_region_grow_amd import render, synthetic

pytestmark = pytest.mark.gpu
SAME_LOGITS_MARGIN = 5e-7      # (test_gpu_grow.py: the same logits on both sides, only exp / divide rounding differs)
W, H = 96, 80


@pytest.fixture(scope='module')
def room():
    return ar.trace_room()


def gpu_net_fn(net):
    def fn(xi, xn):
        _, add, _, rmv, _ = net.run(xi, xn)
        return add, rmv
    return fn


def gpu_visibility(rd, mat=None):
    import torch
    if mat is None:
        rd.build_visibility()
    torch.cuda.synchronize()
    return rd.d_vis.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize('size', [1, 5])
def test_visibility_of_a_room(cuda_device, room, size):
    _, xyz, uneq = room
    assert len(xyz) % 64 and len(xyz) > 1024                              # several blocks, a ragged last wavefront
    rd = render.Renderer(xyz, uneq, int(uneq.max()) + 1, W, H, size, device=cuda_device)
    got = gpu_visibility(rd)
    want = ar.visibility(xyz, ar.camera_matrix(W, H), W, H, size)
    assert (want != ar.EMPTY).sum() > 64 and (want == ar.EMPTY).any()      # (thousands of points on a hundred-odd pixels: every pixel is fought over)
    assert np.array_equal(got, want)


def crafted_cloud():
    """Exact duplicates, points on each clip plane, behind the eye, at the window's corners, non-finite ones."""
    m = ar.camera_matrix(W, H).astype(np.float64)
    inv = np.linalg.inv(m)
    pts = []
    for ndc in ([-1, 0, 0], [1, 0, 0], [0, -1, 0], [0, 1, 0], [0, 0, -1], [0, 0, 1], [-1, -1, 0.5], [1, 1, 0.5], [-1, 1, 0.5], [1, -1, 0.5],
                [0.999, 0.999, 0.2], [-0.999, -0.999, 0.2], [1.001, 0, 0], [0, -1.001, 0], [0.3, 0.3, 0.9], [0.3, 0.3, 0.9]):
        p = inv @ np.array(ndc + [1.0])
        pts.append(p[:3] / p[3])
    eye = np.array(ar.EYE)
    pts += [1.5 * eye, 1.0 * eye, 0.95 * eye, 0.5 * eye, 0.5 * eye, np.zeros(3), np.zeros(3), [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]]
    rs = np.random.RandomState(8)
    pts += list(rs.uniform(-6, 6, (40, 3)))
    return np.asarray(pts, dtype=np.float32)


@pytest.mark.parametrize('case', ['crafted', 'one', 'ragged'])
def test_visibility_edge_cases(cuda_device, case):
    xyz = dict(crafted=crafted_cloud(), one=np.zeros((1, 3), np.float32), ragged=np.random.RandomState(2).uniform(-4, 4, (3 * 64 + 17, 3)).astype(np.float32))[case]
    for w, h, size in ((W, H, 5), (40, 96, 3), (97, 33, 1)):
        rd = render.Renderer(xyz, np.zeros(len(xyz), np.int32), 1, w, h, size, device=cuda_device)
        got = gpu_visibility(rd)
        want = ar.visibility(xyz, ar.camera_matrix(w, h), w, h, size)
        assert (want != ar.EMPTY).any()
        assert np.array_equal(got, want), (case, w, h, size)
    with pytest.raises(ValueError):
        render.Renderer(xyz, np.zeros(len(xyz), np.int32), 1, W, H, 4, device=cuda_device)
    import ctypes
    from learn_region_grow_amd import _lib
    m = np.ascontiguousarray(ar.camera_matrix(W, H).reshape(16))
    assert rd.lib.lrg_render_visibility(ctypes.c_void_p(rd.d_xyz.data_ptr()), len(xyz), m.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), w, h, 4,
                                        ctypes.c_void_p(rd.d_vis.data_ptr()), None) == _lib.LRG_EINVAL - 1      # even sizes are refused


@pytest.mark.parametrize('w, h', [(W, H), (97, 33)])
def test_shade_three_frames_with_text(cuda_device, room, w, h):
    """Three frames (step, seg, step), n not a multiple of 4, the highest palette entry (white text) and the highest paint (19) in use,
    the text area included; a width that is no multiple of 4 takes the byte-wide kernel."""
    import torch
    _, xyz, uneq = room
    n = int(uneq.max()) + 1
    assert n % 4
    rd = render.Renderer(xyz, uneq, n, w, h, 3, device=cuda_device)
    rs = np.random.RandomState(4)
    stride = (n + 15) // 16 * 16
    index = np.zeros((3, stride), np.uint8)
    index[0, :n], index[1, :n], index[2, :n] = rs.randint(0, 8, n), rs.randint(0, 20, n), rs.randint(0, 8, n)
    index[1, :40] = 19
    texts = [render.text_lines(7, 12345, 678, 90, 1), None, render.text_lines(1000, 0, 99999999, 3, 3)]
    got = rd.shade(torch.from_numpy(index).to(cuda_device), [0, 1, 0], texts)
    torch.cuda.synchronize()
    want = ar.shade(ar.visibility(xyz, ar.camera_matrix(w, h), w, h, 3), uneq, index, [0, 1, 0], texts, w, h, render.font_table())
    assert (want == ar.WHITE).any() and (want[1] == 19).any() and not (want[1] == ar.WHITE).any() and {ar.GREY, ar.GREEN, ar.BLUE} <= set(np.unique(want[0]))
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.fixture(scope='module')
def traced(cuda_device, room):
    """One room under synthetic weights: the oracle run (GPU logits) of a seed without a near-tie draw, its twin trace, and the GPU's trace."""
    import torch
    from learn_region_grow_amd import trace
    from learn_region_grow_amd.grow import RegionGrower
    from learn_region_grow_amd.lrgnet import LrgNetHIP
    net = LrgNetHIP(1, 1, 512, 512, 13, 0, device=cuda_device).load_weights(synthetic.make_synthetic_weights(**ar.WEIGHT_KW))
    rm, xyz, uneq = room
    runs = {}

    def oracle(seed):
        runs[seed] = step_audit.oracle_run(rm, seed, policy='net', net_fn=gpu_net_fn(net))
        return [runs[seed][0]]
    seed, _ = seed_without_near_tie(oracle, ar.TRACE_SEEDS, SAME_LOGITS_MARGIN)
    res, recs = runs[seed]
    tr = trace.GrowthTrace(trace.make_grower(net, seed=seed), rm, uneq, frames_per_batch=7)
    headers, codes, paints = [], [], []
    for b in tr.batches():
        headers.append(b.headers)
        codes.append(b.codes.cpu().numpy())
        paints.append(b.paints.cpu().numpy())
    got = (np.concatenate(headers), np.concatenate(codes), np.concatenate(paints))
    plain = RegionGrower(net, rooms_in_flight=1, rng='counter', seed=seed).run([rm])[0]
    return dict(res=res, recs=recs, want=ar.trace_from_records(rm['points'], recs, res, uneq), got=got, final=tr.result(), plain=plain, calls=tr.calls)


def test_trace_equals_the_twin(traced, room):
    rm = room[0]
    n = len(rm['points'])
    # conditions on the oracle run, not measurements: the room was chosen on the CPU so that they hold (animate_ref.TRACE_ROOM)
    assert ar.trace_conditions(traced['res']) == (True, True, True)
    (gh, gc, gp), (wh, wc, wp) = traced['got'], traced['want']
    print('trace: %d steps in %d host calls, %d regions' % (len(gh), traced['calls'], len(traced['res'].regions)))
    assert len(gh) == len(traced['recs']) == len(wh)                      # one frame per oracle record
    assert (gh[:, 7] == 1).all()
    for k in range(len(wh)):
        assert gh[k, :7].tolist() == wh[k].tolist(), 'step %d: header %s, the twin has %s' % (k, gh[k, :7].tolist(), wh[k].tolist())
        assert np.array_equal(gc[k, :n], wc[k]), 'step %d (seed %d step %d): codes differ at %s' % (k, wh[k, 0], wh[k, 1], np.flatnonzero(gc[k, :n] != wc[k])[:8])
        assert np.array_equal(gp[k, :n], wp[k]), 'step %d: paint differs' % k
    assert not gc[:, n:].any() and not gp[:, n:].any()                    # nothing behind the room's points
    assert wh[:, 5].sum() > 0 and (wc >> 1 & 1).any()


def test_traced_run_grows_what_an_ordinary_run_grows(traced):
    final, plain, res = traced['final'], traced['plain'], traced['res']
    key = lambda x: (x['seed'], x['steps'], x['points'], x['reason'], x['labeled'])
    assert [key(x) for x in final.regions] == [key(x) for x in plain.regions] == [key(x) for x in res.regions]
    assert np.array_equal(final.cluster_label, plain.cluster_label) and np.array_equal(final.filled_label, plain.filled_label)
    assert np.array_equal(final.filled_label, res.filled_label)


def test_trace_refuses_what_it_does_not_follow(cuda_device, room):
    from learn_region_grow_amd import trace
    from learn_region_grow_amd.grow import RegionGrower
    from learn_region_grow_amd.lrgnet import LrgNetHIP
    net = LrgNetHIP(1, 1, 512, 512, 13, 0, device=cuda_device).load_weights(synthetic.make_synthetic_weights(**ar.WEIGHT_KW))
    with pytest.raises(ValueError, match='legacy'):
        trace.GrowthTrace(RegionGrower(net, rooms_in_flight=1, rng='legacy'), room[0])
    with pytest.raises(ValueError, match='greedy'):
        trace.GrowthTrace(RegionGrower(net, rooms_in_flight=1, restarts=3), room[0])


def test_driver_writes_the_twins_frames(cuda_device, room, tmp_path):
    """animate_region_growing.py in a child process on a temporary room file: --size 128 --max-frames 6 -> twelve pictures, each the twin's frame."""
    from learn_region_grow_amd.lrgnet import LrgNetHIP
    raw = synthetic.area5_shaped_room(ar.TRACE_ROOM['n_raw'], ar.TRACE_ROOM['seed'], n_furniture=ar.TRACE_ROOM['n_furniture']).astype(np.float32)
    h5 = str(tmp_path / 'rooms.h5')
    lio.saveToH5(h5, [raw])
    rm, xyz, uneq = room
    rm = dict(rm, room_id=0)                                              # the driver keys the stream by the room's index in the file
    runs = {}

    def oracle(seed):                                                     # the driver's synthetic weights are seeded by --seed too
        net = LrgNetHIP(1, 1, 512, 512, 13, 0, device=cuda_device).load_weights(synthetic.make_synthetic_weights(seed=seed, feature_size=13, lite=0))
        runs[seed] = step_audit.oracle_run(rm, seed, policy='net', net_fn=gpu_net_fn(net))
        return [runs[seed][0]]
    seed, _ = seed_without_near_tie(oracle, range(3, 11), SAME_LOGITS_MARGIN)
    res, recs = runs[seed]
    assert len(recs) >= 6
    out = str(tmp_path / 'frames')
    run = subprocess.run([sys.executable, os.path.join(REPO, 'animate_region_growing.py'), '--h5', h5, '--room', '0', '--synthetic-weights', '--seed', str(seed),
                          '--size', '128', '--max-frames', '6', '--frames-per-batch', '4', '--out', out], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert run.returncode == 0, run.stdout + run.stderr
    assert sorted(os.listdir(out)) == sorted(['%s%03d.png' % (k, i) for k in ('step', 'seg') for i in range(6)])
    headers, codes, paints = ar.trace_from_records(rm['points'], recs, res, uneq)
    vis = ar.visibility(xyz, ar.camera_matrix(128, 128), 128, 128, 5)
    index = np.concatenate([codes[:6], paints[:6]])
    want = ar.shade(vis, uneq, index, [0] * 6 + [1] * 6, [ar.text_lines(h) for h in headers[:6]] + [None] * 6, 128, 128, render.font_table())
    pal = render.palette()
    for i in range(6):
        assert np.array_equal(lio.read_png(os.path.join(out, 'step%03d.png' % i)), pal[want[i]]), 'step%03d.png' % i
        assert np.array_equal(lio.read_png(os.path.join(out, 'seg%03d.png' % i)), pal[want[6 + i]]), 'seg%03d.png' % i
    assert (want[:6] == ar.WHITE).any() and (want[:6] == ar.BLUE).any() and (want[6:] != want[:6]).any()
    assert 'points (%d, 13)' % len(rm['points']) in run.stdout
