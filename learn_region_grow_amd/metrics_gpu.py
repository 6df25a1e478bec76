"""The evaluation block of all rooms of a call in one device pass (C-ABI ``lrg_metrics_batch``; the reference blocks are
test_region_grow.py:319-355 and test_mcpnet.py:146-170, the host version is ``metrics.room_metrics`` / ``room_metrics_set_order``).

The split.  The device makes what is large and regular: the contingency tables, the integer sums, the entropies / mutual information /
expected mutual information with sklearn's arithmetic, the greedy matching and ``cluster_label2``.  The host keeps what is NumPy / Python
behaviour or needs wide integers: ``numpy.unique`` of the ground truth and the two visit orders (``prepare_ground_truth``, once per room,
possible before growing), and the finish from the device's scalars with the very expressions of ``metrics.py`` and sklearn
(``scores_from_sums``: the adjusted Rand score's products overflow int64 at 100 k points, so they are Python integers).

``room_metrics_batch`` returns dicts with the keys of ``metrics.room_metrics``: prc / rcl / iou / cluster_label2 equal the host's bit for
bit, ars equals sklearn's, nmi / ami agree with sklearn's to ~1e-10 (a different lgamma and another summation order).
"""
import ctypes
import time

import numpy as np

from . import _lib

EPS = float(np.finfo('float64').eps)
INT_SUMS, FLOAT_SUMS = 8, 4         # csrc/lrg_metrics.hip: MT_ISUMS, MT_FSUMS


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def prepare_ground_truth(obj_id, order='size'):
    """The ground-truth side of one room, from obj_id alone: gt_row (the return_inverse of numpy.unique), the visit order of the GT rows
    and the value a cluster matched at visit k receives.  order='size': numpy.argsort(count)[::-1] and k + 1 (test_region_grow.py:327,:336);
    order='set': ``for i in set(obj_id)`` and i (test_mcpnet.py:152,:160)."""
    obj_id = np.asarray(obj_id)
    if obj_id.ndim != 1 or len(obj_id) == 0:
        raise ValueError('obj_id must be a non-empty 1-D array')
    unique_id, inv, count = np.unique(obj_id, return_inverse=True, return_counts=True)
    if order == 'size':
        visit = np.argsort(count)[::-1]
        relabel = np.arange(1, len(unique_id) + 1)
    elif order == 'set':
        row = {v: g for g, v in enumerate(unique_id.tolist())}
        ids = set(obj_id)                      # numpy scalars, as the reference has them: their hash order is the visit order
        visit = np.array([row[int(i)] for i in ids])
        relabel = np.array([int(i) for i in ids])
    else:
        raise ValueError(order)
    base = int(obj_id.max())
    if len(obj_id) + abs(base) >= 2 ** 31 or np.abs(relabel).max() >= 2 ** 31:
        raise ValueError('object ids past int32')
    return dict(n=len(obj_id), n_gt=len(unique_id), gt_row=inv.reshape(-1).astype(np.int32), order=visit.astype(np.int32),
                relabel=relabel.astype(np.int32), unmatched_base=base)


def scores_from_sums(sum_nij2, sum_a2, sum_b2, n, rows, cols, h_true, h_pred, mi, emi):
    """nmi / ami / ars from a room's sums with sklearn's own expressions (normalized_mutual_info_score, adjusted_mutual_info_score with
    its eps clamps, adjusted_rand_score over pair_confusion_matrix).  rows / cols: the labels that occur on either side."""
    sum_nij2, sum_a2, sum_b2, n = int(sum_nij2), int(sum_a2), int(sum_b2), int(n)
    tp = sum_nij2 - n
    fp = sum_b2 - sum_nij2
    fn = sum_a2 - sum_nij2
    tn = n * n - fp - fn - sum_nij2
    if fn == 0 and fp == 0:
        ars = 1.0
    else:
        ars = 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    if rows == 1 and cols == 1:
        return dict(nmi=1.0, ami=1.0, ars=ars)
    if rows == 1 or cols == 1:                                # mutual_info_score and entropy return 0.0 for a single label
        return dict(nmi=0.0, ami=0.0, ars=ars)
    mi = float(np.clip(mi, 0.0, None))
    normalizer = np.mean([h_true, h_pred])
    nmi = 0.0 if mi == 0 else float(mi / normalizer)
    denominator = normalizer - emi
    if denominator < 0:
        denominator = min(denominator, -EPS)
    else:
        denominator = max(denominator, EPS)
    numerator = mi - emi
    if numerator < 0:
        numerator = min(numerator, -EPS)
    else:
        numerator = max(numerator, EPS)
    return dict(nmi=nmi, ami=float(numerator / denominator), ars=ars)


def finish_room(n_cluster, n_gt, dt_match, gt_match, best_iou, cluster_label2, int_sums=None, float_sums=None):
    """A room's dict from the device's outputs, with the expressions of metrics.room_metrics (:342-348)."""
    out = dict(prc=float(np.mean(np.asarray(dt_match, dtype=bool))) if n_cluster else float('nan'),
               rcl=1.0 * int(gt_match) / n_gt,
               iou=float(np.mean(best_iou)),
               cluster_label2=np.asarray(cluster_label2).astype(int))
    if int_sums is not None:
        s = [int(v) for v in int_sums]
        out.update(scores_from_sums(s[0], s[1], s[2], s[3], s[4], s[5], *[float(v) for v in float_sums]))
    return out


def _check_host_labels(cluster_labels):
    """Host label arrays: int32-ready, every value in [0, C] with C the room's maximum.  Returns the per-room maxima (None where the labels
    are a device tensor)."""
    import torch
    ncl = []
    for k, lab in enumerate(cluster_labels):
        if isinstance(lab, torch.Tensor):
            if lab.dim() != 1 or lab.numel() == 0:
                raise ValueError('room %d: cluster labels must be a non-empty 1-D array' % k)
            ncl.append(None)
            continue
        lab = np.asarray(lab)
        if lab.ndim != 1 or len(lab) == 0:
            raise ValueError('room %d: cluster labels must be a non-empty 1-D array' % k)
        if not np.issubdtype(lab.dtype, np.integer):
            raise ValueError('room %d: cluster labels must be integers' % k)
        lo, hi = int(lab.min()), int(lab.max())
        if lo < 0 or hi >= 2 ** 24:
            raise ValueError('room %d: a cluster label outside [0, C] (%d .. %d)' % (k, lo, hi))
        ncl.append(hi)
    return ncl


def run_batch(prepared, cluster_labels, with_scores=True, device=None, n_clusters=None, timing=None):
    """One lrg_metrics_batch over the rooms: ``prepared`` is the list of prepare_ground_truth dicts, ``cluster_labels`` the rooms' labels
    (NumPy arrays or device tensors).  n_clusters: the rooms' C where the caller knows it (default: each room's maximum label; host
    arrays are checked against it with a ValueError).  Returns the device's outputs as NumPy arrays: cluster_label2, best_iou, dt_match,
    gt_match, int_sums, float_sums, status, and the starts (room_start, gt_start, cluster_start, n_cluster)."""
    import torch
    if len(prepared) != len(cluster_labels) or not prepared:
        raise ValueError('need as many label arrays as prepared rooms, and at least one')
    ncl = _check_host_labels(cluster_labels)
    for k, (p, lab) in enumerate(zip(prepared, cluster_labels)):
        if len(lab) != p['n']:
            raise ValueError('room %d: %d labels for %d points' % (k, len(lab), p['n']))
        if n_clusters is not None:
            if ncl[k] is not None and ncl[k] > int(n_clusters[k]):
                raise ValueError('room %d: a cluster label outside [0, C] (%d > %d)' % (k, ncl[k], int(n_clusters[k])))
            ncl[k] = int(n_clusters[k])
    lib = _lib.load()
    if not torch.cuda.is_available():
        raise _lib.LrgHipError('metrics_gpu needs a GPU (use learn_region_grow_amd.metrics on the host)')
    dev = torch.device(device if device is not None else 'cuda:%d' % torch.cuda.current_device())
    clock = time.perf_counter
    spent = {}
    R = len(prepared)
    with torch.cuda.device(dev):
        t0 = clock()
        room_start = np.zeros(R + 1, dtype=np.int32)
        gt_start = np.zeros(R + 1, dtype=np.int32)
        np.cumsum([p['n'] for p in prepared], out=room_start[1:])
        np.cumsum([p['n_gt'] for p in prepared], out=gt_start[1:])
        up = lambda key: torch.from_numpy(np.concatenate([p[key] for p in prepared])).to(dev)      # noqa: E731
        gt_row, order, relabel = up('gt_row'), up('order'), up('relabel')
        base = torch.from_numpy(np.array([p['unmatched_base'] for p in prepared], dtype=np.int32)).to(dev)
        if all(isinstance(lab, torch.Tensor) for lab in cluster_labels):
            labels = torch.cat([lab.to(device=dev, dtype=torch.int32) for lab in cluster_labels])
        elif not any(isinstance(lab, torch.Tensor) for lab in cluster_labels):
            labels = torch.from_numpy(np.concatenate([np.asarray(lab).astype(np.int32) for lab in cluster_labels])).to(dev)
        else:
            labels = torch.cat([lab.to(device=dev, dtype=torch.int32) if isinstance(lab, torch.Tensor) else
                                torch.from_numpy(np.asarray(lab).astype(np.int32)).to(dev) for lab in cluster_labels])
        missing = [k for k in range(R) if ncl[k] is None]
        if missing:                                        # device labels: C is the room's maximum, one copy for all of them
            mx = torch.stack([labels[int(room_start[k]):int(room_start[k + 1])].max() for k in missing]).cpu().numpy()
            for k, v in zip(missing, mx):
                ncl[k] = max(int(v), 0)
        n_cluster = np.array(ncl, dtype=np.int32)
        i32p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))      # noqa: E731
        nbytes = lib.lrg_metrics_batch_workspace_bytes(i32p(room_start), i32p(gt_start), i32p(n_cluster), R)
        if nbytes == 0:
            raise _lib.LrgHipError('lrg_metrics_batch: %d rooms with %d points, %d GT rows and %d clusters do not fit one call'
                                   % (R, room_start[-1], gt_start[-1], int(n_cluster.sum())))
        N, G, C = int(room_start[-1]), int(gt_start[-1]), int(n_cluster.sum())
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        label2 = torch.empty(N, dtype=torch.int32, device=dev)
        best_iou = torch.empty(G, dtype=torch.float64, device=dev)
        dt_match = torch.empty(max(C, 1), dtype=torch.uint8, device=dev)
        gt_match = torch.empty(R, dtype=torch.int32, device=dev)
        isums = torch.empty((R, INT_SUMS), dtype=torch.int64, device=dev)
        fsums = torch.empty((R, FLOAT_SUMS), dtype=torch.float64, device=dev)
        torch.cuda.current_stream().synchronize()
        spent['uploads'] = clock() - t0
        t0 = clock()
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        rc = lib.lrg_metrics_batch(_ptr(labels), _ptr(gt_row), _ptr(order), _ptr(relabel), _ptr(base), i32p(room_start), i32p(gt_start),
                                   i32p(n_cluster), R, 0 if with_scores else 1, _ptr(ws), ws.numel(), _ptr(label2), _ptr(best_iou),
                                   _ptr(dt_match), _ptr(gt_match), _ptr(isums), _ptr(fsums), st)
        _lib.check(rc, 'lrg_metrics_batch')
        ev1.record()
        status = (ctypes.c_int32 * R)()
        _lib.check(lib.lrg_metrics_batch_status(_ptr(ws), i32p(room_start), i32p(gt_start), i32p(n_cluster), R, status, st),
                   'lrg_metrics_batch_status')
        spent['device'] = clock() - t0
        spent['device_events'] = ev0.elapsed_time(ev1) * 1e-3
        t0 = clock()
        out = dict(cluster_label2=label2.cpu().numpy(), best_iou=best_iou.cpu().numpy(), dt_match=dt_match[:C].cpu().numpy(),
                   gt_match=gt_match.cpu().numpy(), int_sums=isums.cpu().numpy(), float_sums=fsums.cpu().numpy(),
                   status=np.array(list(status), dtype=np.int32), room_start=room_start, gt_start=gt_start,
                   cluster_start=np.concatenate(([0], np.cumsum(n_cluster))).astype(np.int64), n_cluster=n_cluster)
        spent['downloads'] = clock() - t0
    if timing is not None:
        for key, v in spent.items():
            timing[key] = timing.get(key, 0.0) + v
    return out


def finish_batch(raw, with_scores=True):
    """The rooms' dicts from run_batch's arrays."""
    out = []
    for k in range(len(raw['n_cluster'])):
        s0, s1 = int(raw['room_start'][k]), int(raw['room_start'][k + 1])
        g0, g1 = int(raw['gt_start'][k]), int(raw['gt_start'][k + 1])
        c0, c1 = int(raw['cluster_start'][k]), int(raw['cluster_start'][k + 1])
        out.append(finish_room(c1 - c0, g1 - g0, raw['dt_match'][c0:c1], raw['gt_match'][k], raw['best_iou'][g0:g1],
                               raw['cluster_label2'][s0:s1], raw['int_sums'][k] if with_scores else None,
                               raw['float_sums'][k] if with_scores else None))
    return out


def room_metrics_batch(obj_ids, cluster_labels, order='size', with_scores=True, device=None, stream=None, prepared=None, timing=None):
    """All rooms in one device pass: a list of dicts with the keys of metrics.room_metrics (prc rcl iou cluster_label2, and nmi ami ars
    with with_scores).  order='size' is metrics.room_metrics, 'set' metrics.room_metrics_set_order.  Labels may be NumPy arrays or device
    tensors; host arrays are range-checked here (ValueError), device tensors by the library (LrgHipError naming the rooms).
    ``prepared``: the rooms' prepare_ground_truth dicts where the caller made them earlier (obj_ids is then not read).
    ``stream``: a torch.cuda.Stream to enqueue on (default: the current one).  ``timing`` collects 'prepare', 'uploads', 'device',
    'device_events', 'downloads' and 'finish' in seconds."""
    import torch
    clock = time.perf_counter
    t0 = clock()
    if prepared is None:
        prepared = [prepare_ground_truth(o, order) for o in obj_ids]
    t_prep = clock() - t0
    if stream is not None:
        with torch.cuda.stream(stream):
            raw = run_batch(prepared, cluster_labels, with_scores, device, timing=timing)
    else:
        raw = run_batch(prepared, cluster_labels, with_scores, device, timing=timing)
    bad = [k for k in range(len(prepared)) if raw['status'][k]]
    if bad:
        raise _lib.LrgHipError('room %s: a cluster label outside [0, C]' % ', '.join(str(b) for b in bad))
    t0 = clock()
    out = finish_batch(raw, with_scores)
    if timing is not None:
        timing['prepare'] = timing.get('prepare', 0.0) + t_prep
        timing['finish'] = timing.get('finish', 0.0) + clock() - t0
    return out
