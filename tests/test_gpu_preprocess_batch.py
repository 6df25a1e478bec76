"""GPU: all rooms of a file in one device pass (lrg_preprocess_batch, preprocess_gpu.preprocess_rooms).  The single-room entries
(lrg_preprocess, preprocess_gpu.preprocess_room) are the same pipeline with one room, so "the batch equals every room alone, bit for
bit" is the room-isolation test, not an independent yardstick.  The independent ones: the digests of everything lrg_preprocess wrote
when it still had launches of its own (tests/golden/preprocess_single_room.json, tools/prep_golden_digests.py), and the oracle loop."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from learn_region_grow_amd import checkpoint, synthetic
from learn_region_grow_amd import io as lio
from oracle import preprocess_ref
import prep_fixtures as P
from prep_fixtures import _ptr, raw_room, six_rooms
from prep_fixtures import capi_single as _capi_single

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('points', 'obj_id', 'cls_id', 'curvatures', 'order', 'equalized_idx', 'unequalized_idx')
MODES = {'lapack': 0, 'jacobi': 1, 'exact': 2}


def _same(got, want, keys=KEYS, what=''):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, want[k].dtype, got[k].shape, want[k].shape)
        np.testing.assert_array_equal(got[k], want[k], err_msg='%s %s' % (what, k))           # (NaN == NaN)


class Batch:
    """The buffers of one lrg_preprocess_batch call."""

    def __init__(self, lib, dev, rooms, F):
        import torch
        self.lib, self.F, self.R = lib, F, len(rooms)
        sizes = [len(r[0]) for r in rooms]
        self.raw_start = np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)
        self.M = M = int(self.raw_start[-1])
        self.raw = torch.from_numpy(np.ascontiguousarray(np.concatenate([r[0][:, :6] for r in rooms]), np.float32)).to(dev)
        self.obj = torch.from_numpy(np.concatenate([np.asarray(r[1], np.int32) for r in rooms])).to(dev)
        self.cls = torch.from_numpy(np.concatenate([np.asarray(r[2], np.int32) for r in rooms])).to(dev)
        self.ws = torch.empty(lib.lrg_preprocess_batch_workspace_bytes(self.rs(), self.R), dtype=torch.uint8, device=dev)
        self.eq, self.uneq, self.obj_o, self.cls_o, self.nflag = (torch.empty(M, dtype=torch.int32, device=dev) for _ in range(5))
        self.eq_start = torch.empty(self.R + 1, dtype=torch.int32, device=dev)
        self.pts = torch.empty((M, F), dtype=torch.float32, device=dev)
        self.curv = torch.empty(M, dtype=torch.float64, device=dev)
        self.cov = torch.empty((M, 9), dtype=torch.float64, device=dev)
        self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def rs(self, raw_start=None):
        self._rs = np.ascontiguousarray(self.raw_start if raw_start is None else raw_start, np.int32)
        return self._rs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))

    def call(self, mode, raw_start=None, n_rooms=None, eq_start=True, ws_bytes=None):
        return self.lib.lrg_preprocess_batch(_ptr(self.raw), 6, _ptr(self.obj), _ptr(self.cls), self.rs(raw_start), self.R if n_rooms is None else n_rooms,
                                             ctypes.c_float(0.1), self.F, mode, _ptr(self.ws), self.ws.numel() if ws_bytes is None else ws_bytes,
                                             _ptr(self.pts), _ptr(self.obj_o), _ptr(self.cls_o), _ptr(self.curv), _ptr(self.eq), _ptr(self.uneq),
                                             _ptr(self.cov), _ptr(self.eq_start) if eq_start else None, _ptr(self.nflag), self.st)

    def status(self):
        got = (ctypes.c_int32 * self.R)()
        assert self.lib.lrg_preprocess_batch_status(_ptr(self.ws), self.rs(), self.R, got, self.st) == 0
        return list(got)

    def rooms(self, mode):
        es = self.eq_start.cpu().numpy()
        out = []
        for r in range(self.R):
            a, b, s0, s1 = int(es[r]), int(es[r + 1]), int(self.raw_start[r]), int(self.raw_start[r + 1])
            d = dict(eq=self.eq[a:b], uneq=self.uneq[s0:s1], cov=self.cov[a:b])
            if mode:
                d.update(points=self.pts[a:b], obj=self.obj_o[a:b], cls=self.cls_o[a:b], curv=self.curv[a:b])
            if mode == 2:
                d['unsafe'] = self.nflag[a:b]
            out.append({k: v.cpu().numpy() for k, v in d.items()})
        return out


@pytest.fixture(scope='module')
def rooms6():
    return six_rooms()


@pytest.mark.parametrize('F', [6, 9, 12, 13])
@pytest.mark.parametrize('eig', ['lapack', 'jacobi', 'exact'])
def test_batch_equals_the_single_room_entry(cuda_device, hip_lib, rooms6, eig, F):
    """Six rooms in one pass, two of them the same room: every output of every room is what the room gives alone -- through the
    wrapper, and at the C-ABI (covariances, un-normalised curvatures and flags included)."""
    from learn_region_grow_amd import preprocess_gpu
    got = preprocess_gpu.preprocess_rooms(rooms6, feature_size=F, eig=eig, device=cuda_device)
    assert len(got) == len(rooms6)
    for k, room in enumerate(rooms6):
        want = preprocess_gpu.preprocess_room(*room, feature_size=F, eig=eig, device=cuda_device)
        assert set(got[k]) == set(want)
        _same(got[k], want, what='room %d' % k)
        if eig == 'exact':
            assert got[k]['exact_stats'] == want['exact_stats']
    mode = MODES[eig]
    b = Batch(hip_lib, cuda_device, rooms6, F)
    assert b.call(mode) == 0
    assert b.status() == [0] * 6
    for k, (g, room) in enumerate(zip(b.rooms(mode), rooms6)):
        w = _capi_single(hip_lib, cuda_device, room, F, mode)
        if mode == 1:
            g.pop('cov'), w.pop('cov')                       # (eig_mode 1 writes no covariances)
        assert set(g) == set(w)
        _same(g, w, keys=sorted(w), what='C-ABI room %d' % k)


def test_digests_of_the_single_room_pipeline(cuda_device, hip_lib, rooms6):
    """Everything lrg_preprocess writes for each of the six rooms (2 500, 2 500, 2 500, 2 500, 1 and 400 raw points), every feature size
    and eig_mode, and the same from room slices of ONE lrg_preprocess_batch call: the sha256 digests recorded from the single-room
    launches before the two pipelines became one.  Bit-exact by construction (nothing written out depends on atomic order); the bits do
    depend on the compiler that builds the library, so the file names it."""
    with open(os.path.join(ROOT, 'tests', 'golden', 'preprocess_single_room.json')) as f:
        gold = json.load(f)
    assert gold['raw_points'] == [len(r[0]) for r in rooms6]
    built = P.hipcc_version()
    note = 'same compiler as recorded' if built == gold['hipcc_version'] else \
        'the library was built by another compiler than the file records (record again with tools/prep_golden_digests.py): %r, recorded %r' % (built, gold['hipcc_version'])
    assert len(gold['digests']) == len(P.DIGEST_F) * len(P.DIGEST_MODES) * 6
    for F in P.DIGEST_F:
        b = Batch(hip_lib, cuda_device, rooms6, F)
        for mode in P.DIGEST_MODES:
            assert b.call(mode) == 0
            for k, (g, room) in enumerate(zip(b.rooms(mode), rooms6)):
                want = gold['digests'][P.digest_key(F, mode, k)]
                w = _capi_single(hip_lib, cuda_device, room, F, mode)
                assert len(w['eq']) == len(g['eq']) == gold['n_equalized'][k]
                assert P.digests(w, mode) == want, ('lrg_preprocess', F, mode, k, note)
                assert P.digests(g, mode) == want, ('lrg_preprocess_batch', F, mode, k, note)


@pytest.fixture(scope='module')
def oracle_rooms():
    rooms = [raw_room(seed) for seed in (1, 2, 5, 7)]
    return rooms, [preprocess_ref.preprocess_room(*r) for r in rooms]


@pytest.mark.parametrize('eig', ['lapack', 'exact'])
def test_batch_against_the_oracle(cuda_device, oracle_rooms, eig):
    from learn_region_grow_amd import preprocess_gpu
    rooms, want = oracle_rooms
    got = preprocess_gpu.preprocess_rooms(rooms, eig=eig, device=cuda_device)
    for g, w in zip(got, want):
        for k in ('points', 'obj_id', 'cls_id', 'equalized_idx', 'unequalized_idx'):
            np.testing.assert_array_equal(g[k], w[k], err_msg=k)
        np.testing.assert_array_equal(g['order'], np.argsort(w['curvatures']))
        if eig == 'exact':
            st = g['exact_stats']
            assert st['lapack_points'] <= 0.15 * st['points'] + 8, st


def test_room_edges_inside_wavefronts_and_scan_blocks(cuda_device):
    """70 rooms of 300 raw points each (sum 21 000): more rooms than a wavefront has lanes, room edges at multiples of 300 -- inside
    wavefronts (64), blocks (256) and scan blocks (2 048).  The batch equals the 70 single calls."""
    from learn_region_grow_amd import preprocess_gpu
    rooms = []
    for seed in range(70):
        rs = np.random.RandomState(100 + seed)
        raw = np.zeros((300, 6), np.float32)
        raw[:, :3] = rs.rand(300, 3) * (0.9, 0.7, 0.5) + rs.randint(-3, 4, 3)
        raw[:, 3:6] = rs.rand(300, 3)
        rooms.append((raw, rs.randint(0, 9, 300), rs.randint(0, 13, 300)))
    got = preprocess_gpu.preprocess_rooms(rooms, eig='exact', device=cuda_device)
    assert len(got) == 70
    for k, room in enumerate(rooms):
        _same(got[k], preprocess_gpu.preprocess_room(*room, eig='exact', device=cuda_device), what='room %d' % k)


def test_chunks_do_not_change_a_bit(cuda_device, rooms6):
    from learn_region_grow_amd import preprocess_gpu
    sizes = [len(r[0]) for r in rooms6]
    sums = sorted({sum(sizes[a:b]) for a in range(6) for b in range(a + 1, 7)})
    budgets = {n: next(m for m in sums if len(preprocess_gpu.plan_chunks(sizes, m)) == n) for n in (1, 3, 6)}
    want = preprocess_gpu.preprocess_rooms(rooms6, eig='exact', device=cuda_device, max_raw_points=budgets[1])
    for n in (3, 6):
        got = preprocess_gpu.preprocess_rooms(rooms6, eig='exact', device=cuda_device, max_raw_points=budgets[n])
        for k in range(6):
            _same(got[k], want[k], what='%d chunks, room %d' % (n, k))
            assert got[k]['exact_stats'] == want[k]['exact_stats']


def test_errors(cuda_device, hip_lib):
    from learn_region_grow_amd import _lib, preprocess_gpu
    rooms = [raw_room(seed, n=600) for seed in (1, 2, 3, 4)]
    far = rooms[2][0].copy()
    far[5, 0] = 3e5
    bad = [rooms[0], rooms[1], (far, rooms[2][1], rooms[2][2]), rooms[3]]
    b = Batch(hip_lib, cuda_device, bad, 13)
    assert b.call(1) == 0
    assert b.status() == [0, 0, 1, 0]                       # the room with the far point, and only it
    with pytest.raises(_lib.LrgHipError, match='room 2'):
        preprocess_gpu.preprocess_rooms(bad, device=cuda_device)
    with pytest.raises(_lib.LrgHipError, match='room 2'):
        preprocess_gpu.preprocess_rooms(bad, device=cuda_device, max_raw_points=1)          # (its position in the list, not in the chunk)
    with pytest.raises(ValueError):
        preprocess_gpu.preprocess_rooms([rooms[0], (rooms[1][0][:0], rooms[1][1][:0], rooms[1][2][:0])], device=cuda_device)
    # refused before anything is launched, each with its own code
    E = _lib.LRG_EINVAL
    rs = b.raw_start
    assert b.call(1, n_rooms=0) == E - 60
    assert b.call(1, raw_start=[0, rs[2], rs[1], rs[3], rs[4]]) == E - 61
    assert b.call(1, raw_start=[0, rs[1], rs[1], rs[3], rs[4]]) == E - 62
    assert b.call(1, eq_start=False) == E - 65
    assert b.call(1, ws_bytes=b.ws.numel() - 1) == E - 66
    wb = hip_lib.lrg_preprocess_batch_workspace_bytes
    assert wb(b.rs(), 4) == b.ws.numel() > 0
    assert wb(b.rs(), 0) == 0 and wb(None, 4) == 0
    assert wb(b.rs([0, rs[2], rs[1], rs[3], rs[4]]), 4) == 0 and wb(b.rs([0, rs[1], rs[1], rs[3], rs[4]]), 4) == 0
    assert wb(b.rs([1, rs[1], rs[2], rs[3], rs[4]]), 4) == 0
    assert wb(b.rs([0, 1 << 30]), 1) == 0 and wb(b.rs([0, 1 << 29]), 1) == 0          # sum M, and the hash segments, past int32


def test_single_room_entry_codes_and_status(cuda_device, hip_lib):
    """lrg_preprocess is the batch with one room and keeps its own codes, in its own precedence; its status is the room's word."""
    import torch
    from learn_region_grow_amd import _lib
    E = _lib.LRG_EINVAL
    raw_np, _, _ = raw_room(1, n=600)
    far_np = raw_np.copy()
    far_np[5, 0] = 3e5
    M, dev = len(raw_np), cuda_device
    nbytes = hip_lib.lrg_preprocess_workspace_bytes(M)
    assert nbytes > 0 and hip_lib.lrg_preprocess_workspace_bytes(0) == 0 and hip_lib.lrg_preprocess_workspace_bytes(1 << 29) == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    eq, uneq, n_dev, obj_o, cls_o = (torch.empty(M, dtype=torch.int32, device=dev) for _ in range(5))
    pts = torch.empty((M, 13), dtype=torch.float32, device=dev)
    curv = torch.empty(M, dtype=torch.float64, device=dev)
    cov = torch.empty((M, 9), dtype=torch.float64, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(raw, n_raw=M, eq=eq, ws_bytes=nbytes, mode=1):
        return hip_lib.lrg_preprocess(_ptr(raw), 6, None, None, n_raw, ctypes.c_float(0.1), 13, mode, _ptr(ws), ws_bytes, _ptr(pts), _ptr(obj_o),
                                      _ptr(cls_o), _ptr(curv), _ptr(eq), _ptr(uneq), _ptr(cov), _ptr(n_dev), st)

    def status():
        got = ctypes.c_int32(-1)
        assert hip_lib.lrg_preprocess_status(_ptr(ws), M, ctypes.byref(got), st) == 0
        return got.value
    raw, far = torch.from_numpy(raw_np).to(dev), torch.from_numpy(far_np).to(dev)
    # refused before anything is launched
    assert call(raw, n_raw=0) == E - 50
    assert call(raw, n_raw=1 << 29) == E - 51
    assert call(raw, eq=None) == E - 52
    assert call(raw, ws_bytes=nbytes - 1) == E - 53
    assert call(raw, mode=3) == E - 56
    assert call(raw, n_raw=0, eq=None, mode=3) == E - 50 and call(raw, eq=None, ws_bytes=nbytes - 1, mode=3) == E - 52       # precedence
    # the room with the far point, then a clean room on the same workspace
    assert call(far) == 0 and status() == 1
    assert call(raw) == 0 and status() == 0


def test_same_batch_twice_same_bits(cuda_device, hip_lib, rooms6):
    """Which slot of its room's table a voxel lands in depends on the order the lanes arrive; nothing that is written out does."""
    b = Batch(hip_lib, cuda_device, rooms6, 13)
    assert b.call(2) == 0
    first = b.rooms(2)
    b.ws.fill_(0x5a)
    assert b.call(2) == 0
    for g, w in zip(b.rooms(2), first):
        _same(g, w, keys=sorted(w))


def test_cli_batched_preprocessing_gives_the_host_labels(cuda_device, tmp_path):
    """region_grow.py --preprocess gpu-exact (the rank's rooms in one batch) prints the lines of --preprocess host and saves the same clouds."""
    raw = [synthetic.generate_room_points(700 + 200 * i, 90 + i, wlh=(1.2 + 0.15 * i, 1.1, 1.0)).astype(np.float32) for i in range(3)]
    h5 = str(tmp_path / 'rooms.h5')
    lio.saveToH5(h5, raw)
    prefix = str(tmp_path / 'lrgnet.ckpt')
    checkpoint.write_bundle(prefix, synthetic.make_synthetic_weights(seed=0, gain=2.0, bias_std=0.2, add_bias_shift=0.0, rmv_bias_shift=-3.0))
    outs = {}
    for mode in ('gpu-exact', 'host'):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'region_grow.py'), '--h5', h5, '--ckpt', prefix, '--policy', 'gt', '--seed', '5',
                            '--preprocess', mode, '--save', str(tmp_path / mode)], capture_output=True, text=True, cwd=str(tmp_path), timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[mode] = [ln for ln in r.stdout.splitlines() if ln.startswith(('room ', 'Area '))]
    assert len(outs['host']) > 3 and outs['gpu-exact'] == outs['host']
    for i in range(3):
        assert open(str(tmp_path / 'gpu-exact' / ('%d.ply' % i))).read() == open(str(tmp_path / 'host' / ('%d.ply' % i))).read()
