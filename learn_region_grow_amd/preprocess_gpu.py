"""Room preprocessing P0 on the GPU (C-ABI ``lrg_preprocess_batch``; the reference block is test_region_grow.py:119-173).

``preprocess_room`` has the signature and return dict of ``preprocess.preprocess_room`` (the host NumPy version).

eig='lapack'  the GPU does equalisation, neighbour gathering and the float64 covariances (bit-identical to the reference
              loop); the 3x3 SVDs run through ``numpy.linalg.svd`` on the host exactly as the reference calls it.  Every
              output equals the host version bit for bit.
eig='jacobi'  everything on the GPU (Jacobi eigen-solve in float64); features agree with the reference to float32
              rounding and the seed order up to ties / differences below ~1e-13 in curvature.
eig='exact'   the Jacobi solve on the GPU, VERIFIED: both solvers are backward stable, so their singular values of one matrix differ by a
              few eps |cov| and their vectors by that over the gap to the next singular value.  With a slack of 256 eps (EXACT_SLACK)
              a float32 feature whose rounding is the same at both ends of its interval, and a curvature further than the slack from
              its neighbours in the seed order, are what LAPACK would have given; the points that fail either test (near-degenerate
              neighbourhoods, values next to a float32 rounding boundary, ties, the candidates for the maximum curvature: a few per
              thousand) are redone with ``numpy.linalg.svd`` on the host exactly as the reference calls it.  ``points`` and ``order`` --
              everything the region-grow loop reads -- equal the host version bit for bit; ``curvatures`` (float64, not read by the
              loop) are LAPACK's where redone and within 1e-13 elsewhere.  The all-GPU rate instead of a host decomposition per point.

There is one pipeline: ``preprocess_rooms`` takes a list of rooms, and ``preprocess_room`` is a chunk of one room.  The rooms of a chunk (``plan_chunks``) go to the
device as one array and through one fixed set of launches, and come back with one copy per output array; the host finishes of 'exact'
and 'lapack' call ``numpy.linalg.svd`` once per pass on the stacked covariances of all rooms.  Every room's dict equals what
the room gives alone, bit for bit.
"""
import ctypes
import time

import numpy as np
import torch

from . import _lib


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


EXACT_SLACK = 256.0 * np.finfo(np.float64).eps      # bound used for |Jacobi - LAPACK| in units of the largest singular value (csrc: PREP_EIG_SLACK)


def _lapack(cov_h):
    """The reference's own calls on a stack of covariances (test_region_grow.py:158-161): |V[2]| and S[2] / sum(S)."""
    _, S, V = np.linalg.svd(cov_h)
    return np.fabs(V[:, 2, :]), np.fabs(S[:, 2] / (S[:, 0] + S[:, 1] + S[:, 2]))


# ---- all rooms of a file in one device pass ----
DEFAULT_MAX_RAW_POINTS = 1 << 22       # raw points per lrg_preprocess_batch call: ~300 bytes of workspace and outputs per raw point on the device


def plan_chunks(sizes, max_raw_points):
    """Consecutive chunks [(first, last + 1), ...] of the rooms whose raw-point counts are `sizes`, each within `max_raw_points` in total;
    a room larger than the budget is a chunk of its own.  Order kept, every room in exactly one chunk."""
    if max_raw_points < 1:
        raise ValueError('max_raw_points must be positive')
    chunks, first, load = [], 0, 0
    for i, m in enumerate(sizes):
        if i > first and load + m > max_raw_points:
            chunks.append((first, i))
            first, load = i, 0
        load += m
    if len(sizes) > first:
        chunks.append((first, len(sizes)))
    return chunks


def exact_finish_batch(eq_start, curv, feats, unsafe, fetch_cov, feature_size, timing=None):
    """The host finish of eig='exact' for the rooms of one batch: Jacobi results from the GPU, the points whose float32 features or seed-order
    position could differ under LAPACK redone with LAPACK -- the decisions room by room, the LAPACK calls once per pass on the covariances
    of all rooms.  NumPy in, NumPy out -- no GPU needed:

    eq_start [R + 1]        equalised rows of room r are eq_start[r] .. eq_start[r + 1] of everything below
    curv [N] float64        un-normalised S[2] / sum(S) of the device solve (not modified)
    feats [N, F] float32    the device's feature rows (normals from the device solve); modified in place and returned in slices
    unsafe [N]              the device's flags (csrc: PREP_EIG_SLACK rule)
    fetch_cov(idx)          covariances [len(idx), 3, 3] (or [len(idx), 9]) float64 of the batch-wide row numbers idx (int64, ascending)

    Returns one dict per room: points, curvatures, order, exact_stats."""
    F = feature_size
    eq_start = np.asarray(eq_start, dtype=np.int64)
    R, N = len(eq_start) - 1, int(eq_start[-1])
    c = np.array(curv[:N], dtype=np.float64)
    unsafe = np.asarray(unsafe[:N]).astype(bool)
    exact = np.zeros(N, dtype=bool)
    clock = time.perf_counter

    def spend(key, t0):
        if timing is not None:
            timing[key] = timing.get(key, 0.0) + clock() - t0

    def redo_points(mask):
        idx = np.nonzero(mask & ~exact)[0]
        if len(idx) == 0:
            return
        cov_h = np.asarray(fetch_cov(idx)).reshape(-1, 3, 3)
        t0 = clock()
        nrm, cc = _lapack(cov_h)
        spend('lapack', t0)
        c[idx] = cc
        if F >= 12:
            feats[idx, 9:12] = nrm.astype(np.float32)
        exact[idx] = True

    bounds = [(int(eq_start[r]), int(eq_start[r + 1])) for r in range(R)]
    redo = np.zeros(N, dtype=bool)
    for a, b in bounds:
        cr = c[a:b]
        if not np.isfinite(cr).all():                        # degenerate room (a NaN curvature poisons the maximum, :163): every point through LAPACK
            redo[a:b] = True
        else:
            redo[a:b] = unsafe[a:b] | (cr >= cr.max() - 2.0 * EXACT_SLACK)        # ... and whoever could be the maximum
    redo_points(redo)
    stats = [dict(points=b - a, first_pass=int(exact[a:b].sum())) for a, b in bounds]
    again = np.zeros(N, dtype=bool)
    cmaxs = []
    for a, b in bounds:
        cr, ex = c[a:b], exact[a:b]
        cmax = cr[ex].max() if ex.any() else cr.max()       # LAPACK's maximum: the true one is among the candidates
        cmaxs.append(cmax)
        cn = cr / cmax
        dn = np.where(ex, 0.0, EXACT_SLACK / cmax * (1.0 + 1e-9))
        amb = (cn - dn).astype(np.float32) != (cn + dn).astype(np.float32)
        t0 = clock()
        s = np.argsort(cn)
        spend('argsort', t0)
        # neighbours in the seed order closer than TWICE the sum of their slacks: after the redo a point has moved by at most its slack, and
        # the true value of an untouched neighbour lies within its own -- what is left of the gap keeps every pair's order
        close = np.diff(cn[s]) <= 2.0 * (dn[s][1:] + dn[s][:-1])
        near = np.zeros(b - a, dtype=bool)
        near[s[1:][close]] = True
        near[s[:-1][close]] = True
        again[a:b] = (amb | near) & ~ex
    redo_points(again)
    out = []
    for (a, b), cmax, st in zip(bounds, cmaxs, stats):
        cn = c[a:b] / cmax
        st['lapack_points'] = int(exact[a:b].sum())
        if F >= 13:
            feats[a:b, 12] = cn.astype(np.float32)
        t0 = clock()
        order = np.argsort(cn)
        spend('argsort', t0)
        out.append(dict(points=feats[a:b], curvatures=cn, order=order, exact_stats=st))
    return out


def _preprocess_chunk(lib, dev, rooms, first_room, resolution, F, mode, timing, single=False):
    """The rooms of one lrg_preprocess_batch call, start to finish.  single: the call is preprocess_room's (errors name no room)."""
    clock = time.perf_counter
    t_begin = clock()
    sizes = [len(p) for p, _, _ in rooms]
    for k, m in enumerate(sizes):
        if m == 0:
            raise ValueError('empty room (room %d)' % (first_room + k))
    R, M = len(rooms), int(sum(sizes))
    raw_start = np.zeros(R + 1, dtype=np.int32)
    np.cumsum(sizes, out=raw_start[1:])
    raw_np, obj_np, cls_np = np.empty((M, 6), dtype=np.float32), np.empty(M, dtype=np.int32), np.empty(M, dtype=np.int32)
    for k, (p, o, c) in enumerate(rooms):                    # (each room copied once, to its rows of the batch's arrays)
        s0, s1 = raw_start[k], raw_start[k + 1]
        raw_np[s0:s1] = np.asarray(p)[:, :6]
        obj_np[s0:s1] = o
        cls_np[s0:s1] = c
    rs_p = raw_start.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    nbytes = lib.lrg_preprocess_batch_workspace_bytes(rs_p, R)
    if nbytes == 0:
        raise _lib.LrgHipError('a room of %d raw points is too large for the hash tables' % M if single else
                               'lrg_preprocess_batch: %d rooms with %d raw points do not fit one call (lower max_raw_points)' % (R, M))
    spent = {}
    with torch.cuda.device(dev):
        t0 = clock()
        raw = torch.from_numpy(raw_np).to(dev)        # (the ids stay on the host: every mode gathers them there with equalized_idx)
        spent['copies'] = clock() - t0
        t0 = clock()
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        eq = torch.empty(M, dtype=torch.int32, device=dev)
        uneq = torch.empty(M, dtype=torch.int32, device=dev)
        eqs_dev = torch.empty(R + 1, dtype=torch.int32, device=dev)
        pts = torch.empty((M, F), dtype=torch.float32, device=dev) if mode else None
        curv = torch.empty(M, dtype=torch.float64, device=dev) if mode else None
        cov = torch.empty((M, 9), dtype=torch.float64, device=dev) if mode != 1 else None
        nflag = torch.empty(M, dtype=torch.int32, device=dev) if mode == 2 else None
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = lib.lrg_preprocess_batch(_ptr(raw), 6, None, None, rs_p, R, ctypes.c_float(resolution), F, mode, _ptr(ws), ws.numel(),
                                      _ptr(pts), None, None, _ptr(curv), _ptr(eq), _ptr(uneq), _ptr(cov), _ptr(eqs_dev), _ptr(nflag), st)
        _lib.check(rc, 'lrg_preprocess_batch (one room)' if single else 'lrg_preprocess_batch')
        status = (ctypes.c_int32 * R)()
        _lib.check(lib.lrg_preprocess_batch_status(_ptr(ws), rs_p, R, status, st), 'lrg_preprocess_batch_status')
        spent['device'] = clock() - t0
        bad = [first_room + k for k in range(R) if status[k]]
        if bad:
            raise _lib.LrgHipError('%sa point lies outside the +-2^20 voxel window at resolution %g'
                                   % ('' if single else 'room %s: ' % ', '.join(str(b) for b in bad), resolution))
        t0 = clock()
        eq_start = eqs_dev.cpu().numpy().astype(np.int64)
        N = int(eq_start[-1])
        eq_h = eq[:N].cpu().numpy().astype(np.int64)
        uneq_h = uneq.cpu().numpy().astype(np.int64)
        if mode:
            feats = pts[:N].cpu().numpy()
            c_h = curv[:N].cpu().numpy()
        if mode == 2:
            unsafe_h = nflag[:N].cpu().numpy()
        if mode == 0:
            cov_h = cov[:N].cpu().numpy().reshape(N, 3, 3)
        spent['copies'] += clock() - t0

        def fetch_cov(idx):
            t0 = clock()
            got = cov[torch.from_numpy(idx).to(dev)].cpu().numpy()
            spent['copies'] += clock() - t0
            return got
        if mode == 2:
            fin = exact_finish_batch(eq_start, c_h, feats, unsafe_h, fetch_cov, F, timing=spent)
    out = []
    if mode == 0:
        # ---- host finish, the reference's own calls (:158-172), the decomposition once on the stack of all rooms ----
        t0 = clock()
        _, S_all, V_all = np.linalg.svd(cov_h)
        spent['lapack'] = spent.get('lapack', 0.0) + clock() - t0
    for k in range(R):
        a, b = int(eq_start[k]), int(eq_start[k + 1])
        s0, s1 = int(raw_start[k]), int(raw_start[k + 1])
        equalized_idx, unequalized_idx = eq_h[a:b], uneq_h[s0:s1]
        if mode == 2:
            d = fin[k]
        elif mode == 1:
            c = c_h[a:b]
            t0 = clock()
            order = np.argsort(c)
            spent['argsort'] = spent.get('argsort', 0.0) + clock() - t0
            d = dict(points=feats[a:b], curvatures=c, order=order)
        else:
            points = raw_np[s0:s1][equalized_idx]
            xyz, rgb = points[:, :3], points[:, 3:6]
            room_coordinates = (xyz - xyz.min(axis=0)) / (xyz.max(axis=0) - xyz.min(axis=0))
            S, V = S_all[a:b], V_all[a:b]
            normals = np.fabs(V[:, 2, :])
            c = np.fabs(S[:, 2] / (S[:, 0] + S[:, 1] + S[:, 2]))
            c = c / c.max()
            cols = (xyz, room_coordinates) + ((rgb,) if F >= 9 else ()) + ((normals,) if F >= 12 else ()) + ((c.reshape(-1, 1),) if F >= 13 else ())
            t0 = clock()
            order = np.argsort(c)
            spent['argsort'] = spent.get('argsort', 0.0) + clock() - t0
            d = dict(points=np.hstack(cols).astype(np.float32), curvatures=c, order=order)
        d.update(obj_id=obj_np[s0:s1][equalized_idx], cls_id=cls_np[s0:s1][equalized_idx], equalized_idx=equalized_idx, unequalized_idx=unequalized_idx)
        out.append(d)
    if timing is not None:
        spent['total'] = clock() - t_begin
        for key, v in spent.items():
            timing[key] = timing.get(key, 0.0) + v
    return out


def preprocess_rooms(rooms, resolution=0.1, feature_size=13, eig='jacobi', device='cuda:0', max_raw_points=DEFAULT_MAX_RAW_POINTS, timing=None):
    """`rooms`: a list of (points, obj_id, cls_id).  Returns the list of the dicts preprocess_room returns for each (same keys, dtypes and
    bits), from one lrg_preprocess_batch call per chunk of at most max_raw_points raw points.  `timing` (a dict) collects the seconds
    spent in 'device' (the call up to the status read), 'copies', 'lapack', 'argsort' and 'total'."""
    lib = _lib.load()
    if not torch.cuda.is_available():
        raise _lib.LrgHipError('preprocess_gpu needs a GPU (use learn_region_grow_amd.preprocess on the host)')
    if eig not in ('jacobi', 'lapack', 'exact'):
        raise ValueError(eig)
    if feature_size not in (6, 9, 12, 13):
        raise ValueError(feature_size)
    dev = torch.device(device)
    mode = {'jacobi': 1, 'lapack': 0, 'exact': 2}[eig]
    sizes = [len(p) for p, _, _ in rooms]
    for k, m in enumerate(sizes):
        if m == 0:
            raise ValueError('empty room (room %d)' % k)
    out = []
    for first, last in plan_chunks(sizes, max_raw_points):
        out.extend(_preprocess_chunk(lib, dev, rooms[first:last], first, resolution, feature_size, mode, timing))
    return out


def preprocess_room(unequalized_points, obj_id, cls_id, resolution=0.1, feature_size=13, eig='jacobi', device='cuda:0'):
    """One room: a chunk of one."""
    lib = _lib.load()
    if not torch.cuda.is_available():
        raise _lib.LrgHipError('preprocess_gpu needs a GPU (use learn_region_grow_amd.preprocess on the host)')
    if eig not in ('jacobi', 'lapack', 'exact'):
        raise ValueError(eig)
    if len(unequalized_points) == 0:
        raise ValueError('empty room')
    mode = {'jacobi': 1, 'lapack': 0, 'exact': 2}[eig]
    return _preprocess_chunk(lib, torch.device(device), [(unequalized_points, obj_id, cls_id)], 0, resolution, feature_size, mode, None, single=True)[0]
