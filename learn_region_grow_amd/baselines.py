"""The classical region-growing baselines of the reference's benchmarks.py, on the GPU (C-ABI ``lrg_baseline_segment``).

Modes ``normal``, ``curvature``, ``color``, ``feature`` and ``smoothness`` (benchmarks.py:127-142, 251-416): edges on the
26-neighbour voxel graph of an equalised room by a per-mode predicate, connected components, and the components of more than
``min_cluster_size`` points numbered as the reference numbers them.

``room_features``  equalisation and float64 covariances on the GPU (``lrg_preprocess`` eig_mode 0), then the reference's own
                   ``numpy.linalg.svd`` on the host (benchmarks.py:199-249): normals and UNnormalised curvatures bit for bit.
``segment``        the labels of a batch of rooms from one call.

There is no CPU fallback: without the library or a GPU, ``_lib.LrgHipError`` is raised.
"""
import ctypes

import numpy as np
import torch

from . import _lib

MODES = ('normal', 'curvature', 'color', 'feature', 'smoothness')
_MODE_ID = {m: i for i, m in enumerate(MODES)}          # include/lrg_hip.h: LRG_BASELINE_*
MAX_MIN_CLUSTER_SIZE = 64                               # LRG_BASELINE_MAX_MIN_CLUSTER
_NEEDS_NORMALS = ('normal', 'curvature', 'feature', 'smoothness')
_STATUS = {1: 'a point lies outside the +-2^20 voxel window', 2: 'two points of one room share a voxel (the room is not equalised)',
           4: 'a rank lies outside [0, room size)', 8: 'the smoothness replay stack overflowed'}


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def default_thresholds(mode, area=None):
    """(t1, t2, t3) of benchmarks.py:127-142; t2 / t3 only mean something for 'feature'.  area: the first test area."""
    if mode == 'normal':
        return (0.99, 0.0, 0.0)
    if mode == 'curvature':
        return (0.01, 0.0, 0.0)
    if mode == 'color':
        return (0.005, 0.0, 0.0)
    if mode == 'smoothness':
        return (0.985 if str(area) == 'scannet' else 0.98, 0.0, 0.0)
    if mode == 'feature':
        return (0.98, 0.1, 0.1)
    raise ValueError('unknown baseline mode %r (one of %s)' % (mode, ', '.join(MODES)))


def _device(device):
    if not torch.cuda.is_available():
        raise _lib.LrgHipError('learn_region_grow_amd.baselines needs a GPU (there is no CPU fallback)')
    return torch.device(device if device is not None else 'cuda:0')


def room_features(unequalized_points, resolution=0.1, need_normals=True, device=None):
    """benchmarks.py:199-249 for one room: returns dict(points [N,6] float32 xyzrgb, normals [N,3] float64, curvatures [N] float64
    (not divided by their maximum), rank [N] int32 (position in numpy.argsort(curvatures)), equalized_idx, unequalized_idx).
    With need_normals=False (mode 'color') normals, curvatures and rank are None."""
    lib = _lib.load()
    dev = _device(device)
    raw_np = np.ascontiguousarray(np.asarray(unequalized_points)[:, :6], dtype=np.float32)
    M = len(raw_np)
    if M == 0:
        raise ValueError('empty room')
    with torch.cuda.device(dev):
        raw = torch.from_numpy(raw_np).to(dev)
        zeros = torch.zeros(M, dtype=torch.int32, device=dev)
        ws = torch.empty(lib.lrg_preprocess_workspace_bytes(M), dtype=torch.uint8, device=dev)
        eq = torch.empty(M, dtype=torch.int32, device=dev)
        uneq = torch.empty(M, dtype=torch.int32, device=dev)
        n_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        cov = torch.empty((M, 9), dtype=torch.float64, device=dev)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.lrg_preprocess(_ptr(raw), 6, _ptr(zeros), _ptr(zeros), M, ctypes.c_float(resolution), 13, 0, _ptr(ws), ws.numel(),
                                      None, None, None, None, _ptr(eq), _ptr(uneq), _ptr(cov), _ptr(n_dev), st), 'lrg_preprocess')
        status = ctypes.c_int32(0)
        _lib.check(lib.lrg_preprocess_status(_ptr(ws), M, ctypes.byref(status), st), 'lrg_preprocess_status')
        if status.value:
            raise _lib.LrgHipError('a point lies outside the +-2^20 voxel window at resolution %g' % resolution)
        N = int(n_dev.item())
        equalized_idx = eq[:N].cpu().numpy().astype(np.int64)
        out = dict(points=raw_np[equalized_idx], equalized_idx=equalized_idx, unequalized_idx=uneq.cpu().numpy().astype(np.int64),
                   normals=None, curvatures=None, rank=None)
        if not need_normals:
            return out
        cov_h = cov[:N].cpu().numpy().reshape(N, 3, 3)
    _, S, V = np.linalg.svd(cov_h)                                             # :242-246, the reference's own call
    out['normals'] = np.fabs(V[:, 2, :])
    c = np.fabs(S[:, 2] / (S[:, 0] + S[:, 1] + S[:, 2]))
    out['curvatures'] = c
    rank = np.empty(N, dtype=np.int32)
    rank[np.argsort(c)] = np.arange(N, dtype=np.int32)                        # :383, numpy's default (unstable) sort
    out['rank'] = rank
    return out


def segment(rooms, mode, threshold=None, resolution=0.1, min_cluster_size=10, device=None, thresholds=None, return_counts=False):
    """Labels of every room in ONE lrg_baseline_segment call.

    rooms: list of dicts as ``room_features`` returns them (points; normals / curvatures / rank where the mode reads them).
    threshold overrides the mode's first threshold as --threshold does (:119); thresholds=(t1, t2, t3) sets all three.
    Returns a list of int32 label arrays (0 = no cluster), and the per-room cluster counts with return_counts=True."""
    if mode not in _MODE_ID:
        raise ValueError('unknown baseline mode %r (one of %s)' % (mode, ', '.join(MODES)))
    lib = _lib.load()
    dev = _device(device)
    t = list(thresholds if thresholds is not None else default_thresholds(mode))
    if threshold is not None:
        t[0] = float(threshold)
    if not 1 <= min_cluster_size <= MAX_MIN_CLUSTER_SIZE:
        raise ValueError('min_cluster_size must be in [1, %d]' % MAX_MIN_CLUSTER_SIZE)
    if len(rooms) == 0:
        return ([], np.zeros(0, np.int32)) if return_counts else []
    sizes = [len(r['points']) for r in rooms]
    room_start = np.zeros(len(rooms) + 1, dtype=np.int32)
    room_start[1:] = np.cumsum(sizes)
    n = int(room_start[-1])
    need_n = mode in ('normal', 'feature', 'smoothness')
    need_c = mode in ('curvature', 'feature')

    def cat(key, dtype, width):
        if any(r.get(key) is None for r in rooms):
            raise ValueError("mode %r needs '%s' for every room (room_features(..., need_normals=True))" % (mode, key))
        a = np.concatenate([np.asarray(r[key], dtype=dtype).reshape(-1, width) for r in rooms]) if n else np.zeros((1, width), dtype)
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    with torch.cuda.device(dev):
        pts = cat('points', np.float32, 6)
        normals = cat('normals', np.float64, 3) if need_n else None
        curv = cat('curvatures', np.float64, 1) if need_c else None
        rank = cat('rank', np.int32, 1) if mode == 'smoothness' else None
        ws = torch.empty(max(1, lib.lrg_baseline_workspace_bytes(n, len(rooms), min_cluster_size)), dtype=torch.uint8, device=dev)
        labels = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        counts = torch.empty(len(rooms), dtype=torch.int32, device=dev)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.lrg_baseline_segment(_ptr(pts), 6, room_start.ctypes.data_as(ctypes.c_void_p), len(rooms), ctypes.c_float(resolution),
                                            _MODE_ID[mode], _ptr(normals), _ptr(curv), _ptr(rank), t[0], t[1], t[2], min_cluster_size,
                                            _ptr(ws), ws.numel(), _ptr(labels), _ptr(counts), st), 'lrg_baseline_segment')
        status = ctypes.c_int32(0)
        _lib.check(lib.lrg_baseline_status(_ptr(ws), n, len(rooms), min_cluster_size, ctypes.byref(status), st), 'lrg_baseline_status')
        if status.value:
            raise _lib.LrgHipError('lrg_baseline_segment: ' + '; '.join(v for b, v in _STATUS.items() if status.value & b))
        lab = labels[:n].cpu().numpy()
        cnt = counts.cpu().numpy()
    out = [lab[room_start[r]:room_start[r + 1]] for r in range(len(rooms))]
    return (out, cnt) if return_counts else out
