"""The classical region-growing baselines of the reference's benchmarks.py, on the GPU (C-ABI ``lrg_baseline_segment``).

Modes ``normal``, ``curvature``, ``color``, ``feature`` and ``smoothness`` (benchmarks.py:127-142, 251-416): edges on the
26-neighbour voxel graph of an equalised room by a per-mode predicate, connected components, and the components of more than
``min_cluster_size`` points numbered as the reference numbers them.  Mode ``fpfh`` (:354-367, ``ALL_MODES``) does
the same with Fast Point Feature Histograms, computed here (``fpfh``, C-ABI ``lrg_fpfh``) instead of by PCL's command-line tools
(DESIGN.md §3.15).

``room_features``  equalisation and float64 covariances on the GPU (``lrg_preprocess`` eig_mode 0), then the reference's own
                   ``numpy.linalg.svd`` on the host (benchmarks.py:199-249): normals and UNnormalised curvatures bit for bit.
                   With ``eig='verified'`` the 3x3 decompositions run on the GPU too (``lrg_baseline_eig``) with a bound on every
                   value's distance from LAPACK's; the host redoes only the points without a bound and those whose place in
                   ``numpy.argsort(curvatures)`` is not certain, so ``rank`` is the ``lapack`` route's.
``segment``        the labels of a batch of rooms from one call.  Rooms from ``eig='verified'`` first go through
                   ``lrg_baseline_certify`` with this call's mode and thresholds: the points of every edge whose outcome could differ
                   under LAPACK get LAPACK's features, so the labels are the ``lapack`` route's.

There is no CPU fallback: without the library or a GPU, ``_lib.LrgHipError`` is raised.
"""
import ctypes

import numpy as np
import torch

from . import _lib

MODES = ('normal', 'curvature', 'color', 'feature', 'smoothness')
ALL_MODES = MODES + ('fpfh',)                           # fpfh: its own entry points (lrg_fpfh, lrg_baseline_segment_fpfh), no LRG_BASELINE_* id
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
    if mode == 'fpfh':
        return (0.985, 0.0, 0.0)
    raise ValueError('unknown baseline mode %r (one of %s)' % (mode, ', '.join(ALL_MODES)))


def _device(device):
    if not torch.cuda.is_available():
        raise _lib.LrgHipError('learn_region_grow_amd.baselines needs a GPU (there is no CPU fallback)')
    return torch.device(device if device is not None else 'cuda:0')


EIG_ROUTES = ('lapack', 'verified')


def _lapack(cov):
    """The reference's own calls (benchmarks.py:242-246) on covariances [m, 9]: |V[2]| and |S[2] / sum(S)|, exactly the
    expressions of the 'lapack' route (numpy.linalg.svd decomposes every matrix of a stack by itself)."""
    _, S, V = np.linalg.svd(np.asarray(cov, dtype=np.float64).reshape(-1, 3, 3))
    return np.fabs(V[:, 2, :]), np.fabs(S[:, 2] / (S[:, 0] + S[:, 1] + S[:, 2]))


def _verified_finish(cov_h, normals, c, ns, cs):
    """eig='verified' on the host: LAPACK for the points without a bound, then for both members of every neighbouring pair of the
    sorted curvatures closer than twice the sum of their slacks (a redone point moves by at most its slack and an untouched
    neighbour's true value lies within its own, so what is left of the gap keeps every pair's order: DESIGN.md §3.6), then
    numpy.argsort -- a function of the comparisons' outcomes only -- of the final curvatures.  Arrays are changed in place."""
    N = len(c)

    def redo(mask):
        idx = np.nonzero(mask)[0]
        if len(idx):
            normals[idx], c[idx] = _lapack(cov_h[idx])
            ns[idx] = 0.0
            cs[idx] = 0.0
        return len(idx)
    degenerate = redo(~(np.isfinite(ns) & np.isfinite(cs)))
    s = np.argsort(c)
    cs_s = cs[s]
    close = np.diff(c[s]) <= 2.0 * (cs_s[1:] + cs_s[:-1])
    near = np.zeros(N, dtype=bool)
    near[s[1:][close]] = True
    near[s[:-1][close]] = True
    rank_redone = redo(near & (cs > 0.0))
    rank = np.empty(N, dtype=np.int32)
    rank[np.argsort(c)] = np.arange(N, dtype=np.int32)                        # :383, numpy's default (unstable) sort
    return rank, dict(points=N, rank_redone=rank_redone, degenerate=degenerate)


def room_features(unequalized_points, resolution=0.1, need_normals=True, device=None, eig='lapack'):
    """benchmarks.py:199-249 for one room: returns dict(points [N,6] float32 xyzrgb, normals [N,3] float64, curvatures [N] float64
    (not divided by their maximum), rank [N] int32 (position in numpy.argsort(curvatures)), equalized_idx, unequalized_idx).
    With need_normals=False (mode 'color') normals, curvatures and rank are None.

    eig='lapack' (default): every decomposition by numpy.linalg.svd on the host.  eig='verified': lrg_baseline_eig on the device; the
    dict gains cov [N,9] float64, normal_slack and curv_slack [N] float64 (how far LAPACK's value can lie from the one stored; 0
    where LAPACK made it) and verify_stats = dict(points, rank_redone, degenerate).  rank equals the 'lapack' route's; normals and
    curvatures are LAPACK's only where redone, and ``segment`` completes them for the mode and thresholds it is called with."""
    if eig not in EIG_ROUTES:
        raise ValueError('unknown eig route %r (one of %s)' % (eig, ', '.join(EIG_ROUTES)))
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
        if eig == 'verified':
            nrm_d = torch.empty((N, 3), dtype=torch.float64, device=dev)
            sol = torch.empty((3, N), dtype=torch.float64, device=dev)                # curvatures, normal_slack, curv_slack
            _lib.check(lib.lrg_baseline_eig(_ptr(cov), N, _ptr(nrm_d), _ptr(sol[0]), _ptr(sol[1]), _ptr(sol[2]), st), 'lrg_baseline_eig')
            cov_h = cov[:N].cpu().numpy()
            normals = nrm_d.cpu().numpy()
            c, ns, cs = sol.cpu().numpy()
            c, ns, cs = c.copy(), ns.copy(), cs.copy()
            rank, stats = _verified_finish(cov_h, normals, c, ns, cs)
            out.update(normals=normals, curvatures=c, rank=rank, cov=cov_h, normal_slack=ns, curv_slack=cs, verify_stats=stats)
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


def pcd_roundtrip(a):
    """What a float32 value is after the reference's PCD round trip (benchmarks.py:355: savePCD prints '%f', PCL parses float32):
    float32(float('%f' % v)) for every element.  '%f' rounds the value's exact decimal expansion to six places, half to even;
    double(v) * 1e6 is exact (24 bits times the 14 of 15625, times 2^6), so rint of it is that integer, and dividing it by 1e6 is
    correctly rounded, i.e. the double that float() parses from the string."""
    v = np.asarray(a, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid='ignore'):
        return (np.rint(v * 1e6) / 1e6).astype(np.float32)


def _check_radius(resolution, radius):
    radius = 2 * resolution if radius is None else radius
    if not np.float32(radius) > 0 or np.float32(radius) > np.float32(2) * np.float32(resolution):
        raise ValueError('fpfh: radius %g must lie in (0, 2 * resolution = %g]: neighbours are looked for in the +-2 voxel window' %
                         (radius, 2 * resolution))
    return radius


def fpfh(rooms, resolution=0.1, radius=None, device=None, return_counts=False, lists=True):
    """Fast Point Feature Histograms of every room in ONE lrg_fpfh call (benchmarks.py:355-358 without PCL).

    rooms: dicts as ``room_features(..., need_normals=True)`` returns them.  Points and float32(normals) go through
    ``pcd_roundtrip``; the voxels come from the points as they are.  radius defaults to 2 * resolution (:356) and may not exceed it.
    Returns a list of [N, 33] float32 arrays; with return_counts=True also a list of (counts [N, 33] int32, k [N] int32) per room: the
    pair-feature histograms and the neighbour counts (the point itself included) the descriptor is made of.  lists=True (the
    default: the faster form) makes the gather pass read neighbour lists the pair pass stored, 192 bytes a point;
    lists=False makes it probe the window again: same output."""
    radius = _check_radius(resolution, radius)
    if any(r.get('normals') is None for r in rooms):
        raise ValueError("fpfh needs 'normals' for every room (room_features(..., need_normals=True))")
    if len(rooms) == 0:
        return ([], []) if return_counts else []
    lib = _lib.load()
    dev = _device(device)
    room_start = np.zeros(len(rooms) + 1, dtype=np.int32)
    room_start[1:] = np.cumsum([len(r['points']) for r in rooms])
    n = int(room_start[-1])
    flags = _lib.LRG_FPFH_LISTS if lists else 0

    def up(parts, width, dtype=np.float32):
        a = np.concatenate([np.asarray(p, dtype=dtype).reshape(-1, width) for p in parts]) if n else np.zeros((1, width), dtype)
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    with torch.cuda.device(dev):
        pts = up([np.asarray(r['points'], np.float32)[:, :3] for r in rooms], 3)
        xyz = up([pcd_roundtrip(np.asarray(r['points'])[:, :3]) for r in rooms], 3)
        nrm = up([pcd_roundtrip(np.asarray(r['normals'], dtype=np.float64).astype(np.float32)) for r in rooms], 3)
        ws = torch.empty(max(1, lib.lrg_fpfh_workspace_bytes(n, len(rooms), flags)), dtype=torch.uint8, device=dev)
        counts = torch.zeros((max(n, 1), 33), dtype=torch.int32, device=dev)
        k = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        out = torch.zeros((max(n, 1), 33), dtype=torch.float32, device=dev)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.lrg_fpfh(_ptr(pts), 3, _ptr(xyz), _ptr(nrm), room_start.ctypes.data_as(ctypes.c_void_p), len(rooms),
                                ctypes.c_float(resolution), ctypes.c_float(radius), flags, _ptr(ws), ws.numel(), _ptr(counts), _ptr(k), _ptr(out),
                                st), 'lrg_fpfh')
        status = ctypes.c_int32(0)
        _lib.check(lib.lrg_fpfh_status(_ptr(ws), n, len(rooms), flags, ctypes.byref(status), st), 'lrg_fpfh_status')
        if status.value:
            raise _lib.LrgHipError('lrg_fpfh: ' + '; '.join(v for b, v in _STATUS.items() if status.value & b))
        out, counts, k = out[:n].cpu().numpy(), counts[:n].cpu().numpy(), k[:n].cpu().numpy()
    cut = lambda a: [a[room_start[r]:room_start[r + 1]] for r in range(len(rooms))]
    if return_counts:
        return cut(out), list(zip(cut(counts), cut(k)))
    return cut(out)


def _certify(lib, dev, rooms, room_start, n, mode, t, resolution, min_cluster_size, pts, normals, curv, ws, st, cat):
    """lrg_baseline_certify with THIS call's mode and thresholds, then LAPACK's normals and curvatures (from room['cov']) for the
    flagged points, written into the rooms' arrays with slack 0.  Returns the device normals / curvatures to segment with, the flags
    per room and their counts."""
    ns = cat('normal_slack', np.float64, 1)
    cs = cat('curv_slack', np.float64, 1)
    flags = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    n_flagged = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.check(lib.lrg_baseline_certify(_ptr(pts), 6, room_start.ctypes.data_as(ctypes.c_void_p), len(rooms), ctypes.c_float(resolution),
                                        _MODE_ID[mode], _ptr(normals), _ptr(curv), _ptr(ns), _ptr(cs), t[0], t[1], t[2], min_cluster_size,
                                        _ptr(ws), ws.numel(), _ptr(flags), _ptr(n_flagged), st), 'lrg_baseline_certify')
    total = int(n_flagged.item())
    per_room = [np.zeros(room_start[r + 1] - room_start[r], dtype=bool) for r in range(len(rooms))]
    if total:
        fl = flags[:n].cpu().numpy().astype(bool)
        assert int(fl.sum()) == total
        for r, room in enumerate(rooms):
            per_room[r] = fl[room_start[r]:room_start[r + 1]]
            idx = np.nonzero(per_room[r])[0]
            if len(idx):
                room['normals'][idx], room['curvatures'][idx] = _lapack(np.asarray(room['cov']).reshape(-1, 9)[idx])
                room['normal_slack'][idx] = 0.0
                room['curv_slack'][idx] = 0.0
        if normals is not None:
            normals = cat('normals', np.float64, 3)
        if curv is not None:
            curv = cat('curvatures', np.float64, 1)
    return normals, curv, per_room, np.array([int(f.sum()) for f in per_room], dtype=np.int64)


def segment(rooms, mode, threshold=None, resolution=0.1, min_cluster_size=10, device=None, thresholds=None, return_counts=False,
            return_stats=False):
    """Labels of every room in ONE lrg_baseline_segment call.

    rooms: list of dicts as ``room_features`` returns them (points; normals / curvatures / rank where the mode reads them).
    mode: one of ALL_MODES.  'fpfh' (lrg_baseline_segment_fpfh) reads room['fpfh'] ([N, 33] float32) when EVERY room carries it and
    otherwise computes it with ``fpfh`` at this resolution; rooms from eig='verified' are refused for it (ValueError).
    threshold overrides the mode's first threshold as --threshold does (:119); thresholds=(t1, t2, t3) sets all three.
    Returns a list of int32 label arrays (0 = no cluster), and the per-room cluster counts with return_counts=True.

    When EVERY room carries 'normal_slack' (room_features(..., eig='verified')), lrg_baseline_certify runs first with this mode and
    these thresholds, and the points it flags get LAPACK's normals and curvatures from room['cov'] IN PLACE (room['normals'],
    room['curvatures'], slacks set to 0; 'rank' is left alone: no certified pair changes order), so the labels are those of the
    'lapack' route.  return_stats=True appends dict(flagged=[per-room count], flags=[per-room bool array]) to the result, or None
    for rooms without the key, which take the path they always took."""
    if mode not in ALL_MODES:
        raise ValueError('unknown baseline mode %r (one of %s)' % (mode, ', '.join(ALL_MODES)))
    lib = _lib.load()
    dev = _device(device)
    t = list(thresholds if thresholds is not None else default_thresholds(mode))
    if threshold is not None:
        t[0] = float(threshold)
    if not 1 <= min_cluster_size <= MAX_MIN_CLUSTER_SIZE:
        raise ValueError('min_cluster_size must be in [1, %d]' % MAX_MIN_CLUSTER_SIZE)
    verified = len(rooms) > 0 and all(r.get('normal_slack') is not None for r in rooms)
    if mode == 'fpfh' and any(r.get('normal_slack') is not None for r in rooms):
        raise ValueError("mode 'fpfh' does not take rooms from room_features(..., eig='verified'): the certificate bounds how far an edge of "
                         "the normal and curvature predicates can move under LAPACK's features, and none covers the descriptor, whose bins "
                         "depend on the normals discontinuously; use eig='lapack'")
    stats = None
    if len(rooms) == 0:
        res = ([], np.zeros(0, np.int32)) if return_counts else ([],)
        return res + (None,) if return_stats else (res if return_counts else [])
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
        if mode == 'fpfh':
            if any(r.get('fpfh') is None for r in rooms):                    # computed here unless every room brings its own
                hist = fpfh(rooms, resolution=resolution, device=dev)
            else:
                hist = [r['fpfh'] for r in rooms]
            h = np.concatenate([np.asarray(x, dtype=np.float32).reshape(-1, 33) for x in hist]) if n else np.zeros((1, 33), np.float32)
            h = torch.from_numpy(np.ascontiguousarray(h)).to(dev)
            ws = torch.empty(max(1, lib.lrg_baseline_fpfh_workspace_bytes(n, len(rooms), min_cluster_size)), dtype=torch.uint8, device=dev)
            labels = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
            counts = torch.empty(len(rooms), dtype=torch.int32, device=dev)
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.check(lib.lrg_baseline_segment_fpfh(_ptr(pts), 6, room_start.ctypes.data_as(ctypes.c_void_p), len(rooms), ctypes.c_float(resolution),
                                                     _ptr(h), t[0], min_cluster_size, _ptr(ws), ws.numel(), _ptr(labels), _ptr(counts), st),
                       'lrg_baseline_segment_fpfh')
            return _finish(lib, ws, st, n, rooms, room_start, min_cluster_size, labels, counts, return_counts, return_stats, None,
                           'lrg_baseline_segment_fpfh')
        normals = cat('normals', np.float64, 3) if need_n else None
        curv = cat('curvatures', np.float64, 1) if need_c else None
        rank = cat('rank', np.int32, 1) if mode == 'smoothness' else None
        ws = torch.empty(max(1, lib.lrg_baseline_workspace_bytes(n, len(rooms), min_cluster_size)), dtype=torch.uint8, device=dev)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if verified:
            if need_n or need_c:
                normals, curv, per_room, flagged = _certify(lib, dev, rooms, room_start, n, mode, t, resolution, min_cluster_size, pts,
                                                            normals, curv, ws, st, cat)
            else:                                                   # 'color' reads no solved value: nothing to certify
                per_room = [np.zeros(k, dtype=bool) for k in sizes]
                flagged = np.zeros(len(rooms), dtype=np.int64)
            stats = dict(flagged=flagged, flags=per_room)
        labels = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        counts = torch.empty(len(rooms), dtype=torch.int32, device=dev)
        _lib.check(lib.lrg_baseline_segment(_ptr(pts), 6, room_start.ctypes.data_as(ctypes.c_void_p), len(rooms), ctypes.c_float(resolution),
                                            _MODE_ID[mode], _ptr(normals), _ptr(curv), _ptr(rank), t[0], t[1], t[2], min_cluster_size,
                                            _ptr(ws), ws.numel(), _ptr(labels), _ptr(counts), st), 'lrg_baseline_segment')
        return _finish(lib, ws, st, n, rooms, room_start, min_cluster_size, labels, counts, return_counts, return_stats, stats,
                       'lrg_baseline_segment')


def _finish(lib, ws, st, n, rooms, room_start, min_cluster_size, labels, counts, return_counts, return_stats, stats, what):
    """The status word, then the labels cut into rooms, in the shape ``segment`` returns."""
    status = ctypes.c_int32(0)
    _lib.check(lib.lrg_baseline_status(_ptr(ws), n, len(rooms), min_cluster_size, ctypes.byref(status), st), 'lrg_baseline_status')
    if status.value:
        raise _lib.LrgHipError(what + ': ' + '; '.join(v for b, v in _STATUS.items() if status.value & b))
    lab = labels[:n].cpu().numpy()
    cnt = counts.cpu().numpy()
    out = [lab[room_start[r]:room_start[r + 1]] for r in range(len(rooms))]
    res = (out, cnt) if return_counts else (out,)
    if return_stats:
        return res + (stats,)
    return res if return_counts else out
