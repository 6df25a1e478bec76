"""The edge-classifier baseline of the reference's benchmarks.py (``--mode edge``, :308-353 and :406-436) on the GPU.

The reference classifies every edge of the 26-neighbour voxel graph with a pickled ``sklearn`` 0.19 ``MLPClassifier``
(30-100-50-25-1, relu, logistic), keeps the edges whose probability passes a per-point relative threshold, labels the connected
components, and gives every unlabelled point the label of the first labelled point that a probability-ordered depth-first search
from it reaches.  Here (csrc/lrg_edge.hip):

``load_edge_model``  the eight arrays of the pickle (or of an ``.npz``), read without importing sklearn.
``EdgeModelHIP``     the packed float64 weights on the device.
``logits``           nmin / nmax and z [n, 13] of every room (``lrg_edge_logits``).
``probabilities``    z through ``scipy.special.expit`` on the host (what sklearn calls) or ``lrg_edge_sigmoid`` on the device.
``segment``          the labels of a batch of rooms (``lrg_edge_logits``, the sigmoid, ``lrg_edge_segment``).

There is no CPU fallback: without the library or a GPU, ``_lib.LrgHipError`` is raised.
"""
import ctypes
import io
import pickle

import numpy as np

from . import _lib

LAYERS = (30, 100, 50, 25, 1)
WEIGHT_KEYS = ('W0', 'b0', 'W1', 'b1', 'W2', 'b2', 'W3', 'b3')
SLOTS = 13
SIGMOID_ROUTES = ('host', 'device')
_STATUS = {1: 'a point lies outside the +-2^20 voxel window', 2: 'two points of one room share a voxel (the room is not equalised)',
           4: 'a label chain was not resolved'}


class _Stub(object):
    """What every sklearn class of the pickle becomes: an object that only keeps its __dict__."""

    def __init__(self, *args, **kwargs):
        pass

    def __setstate__(self, state):
        if isinstance(state, dict):
            self.__dict__.update(state)


def _stub_class(module, name):
    return type(str(name), (_Stub,), {'__module__': module, 'pickled_as': '%s.%s' % (module, name)})


def _unpickle(path):
    from joblib import numpy_pickle

    class Unpickler(numpy_pickle.NumpyUnpickler):
        def find_class(self, module, name):
            if module.startswith('sklearn.externals.joblib'):
                module = module[len('sklearn.externals.'):]
            elif module == 'sklearn' or module.startswith('sklearn.'):
                return _stub_class(module, name)
            return super().find_class(module, name)

    with open(path, 'rb') as f:
        data = f.read()
    u = Unpickler(path, io.BytesIO(data), True)
    u.encoding = 'latin1'                           # a Python-2 pickle: its str objects are bytes
    try:
        return u.load()
    except (pickle.UnpicklingError, EOFError, AttributeError, ImportError, IndexError, KeyError, UnicodeDecodeError) as e:
        raise ValueError('%s is not a readable joblib / pickle file: %s' % (path, e))


def _check_arrays(arrs, where):
    if len(arrs) != 8:
        raise ValueError('%s: not a four-layer network (%d weight and bias arrays)' % (where, len(arrs)))
    out = []
    for l in range(4):
        W = np.ascontiguousarray(np.asarray(arrs[2 * l], dtype=np.float64))
        b = np.ascontiguousarray(np.asarray(arrs[2 * l + 1], dtype=np.float64)).reshape(-1)
        if W.shape != (LAYERS[l], LAYERS[l + 1]) or b.shape != (LAYERS[l + 1],):
            raise ValueError('%s: layer %d is %s with bias %s, the edge classifier has %d -> %d (30-100-50-25-1)'
                             % (where, l, W.shape, b.shape, LAYERS[l], LAYERS[l + 1]))
        out += [W, b]
    return out


def load_edge_model(path):
    """The reference's models/edge<AREA>.pkl, or an .npz with W0, b0, ..., W3, b3: the eight float64 arrays [W0, b0, ..., W3, b3]
    (W [in, out]).  The pickle is a Python-2 joblib file of sklearn 0.19's MLPClassifier; it is read with joblib's unpickler, byte
    strings decoded as latin1, ``sklearn.externals.joblib`` mapped to ``joblib`` and every other sklearn class replaced by a stub
    that keeps its attributes, so no sklearn is imported.  ValueError unless the object is a 30-100-50-25-1 network with relu
    hidden layers and a logistic output."""
    path = str(path)
    if path.endswith('.npz'):
        with np.load(path) as z:
            missing = [k for k in WEIGHT_KEYS if k not in z.files]
            if missing:
                raise ValueError('%s lacks %s' % (path, ', '.join(missing)))
            return _check_arrays([z[k] for k in WEIGHT_KEYS], path)
    m = _unpickle(path)
    d = getattr(m, '__dict__', None)
    if not isinstance(d, dict) or 'coefs_' not in d or 'intercepts_' not in d:
        raise ValueError('%s does not hold a multi-layer perceptron (no coefs_ / intercepts_)' % path)
    act, out_act = d.get('activation'), d.get('out_activation_')
    if act != 'relu':
        raise ValueError("%s: hidden activation %r, the edge classifier's is 'relu'" % (path, act))
    if out_act != 'logistic':
        raise ValueError("%s: output activation %r, the edge classifier's is 'logistic'" % (path, out_act))
    coefs, icpt = list(d['coefs_']), list(d['intercepts_'])
    if len(coefs) != len(icpt):
        raise ValueError('%s: %d weight arrays and %d bias arrays' % (path, len(coefs), len(icpt)))
    arrs = []
    for W, b in zip(coefs, icpt):
        arrs += [W, b]
    return _check_arrays(arrs, path)


def pack_weights(weights):
    """W0 | b0 | W1 | b1 | W2 | b2 | W3 | b3 as one float64 vector (LRG_EDGE_WEIGHTS values)."""
    return np.concatenate([a.reshape(-1) for a in _check_arrays(list(weights), 'weights')])


def _torch():
    import torch
    return torch


def _device(device):
    torch = _torch()
    if not torch.cuda.is_available():
        raise _lib.LrgHipError('learn_region_grow_amd.edge needs a GPU (there is no CPU fallback)')
    return torch.device(device if device is not None else 'cuda:0')


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class EdgeModelHIP(object):
    """The classifier's weights on the device.  weights: the eight arrays of ``load_edge_model`` (or a path it reads)."""

    def __init__(self, weights, device=None):
        if isinstance(weights, (str, bytes)) or hasattr(weights, '__fspath__'):
            weights = load_edge_model(weights)
        self.lib = _lib.load()
        self.device = _device(device)
        self.weights = _check_arrays(list(weights), 'weights')
        self.packed = _torch().from_numpy(pack_weights(self.weights)).to(self.device)


def _batch(rooms, dev):
    torch = _torch()
    sizes = [len(r['points']) for r in rooms]
    room_start = np.zeros(len(rooms) + 1, dtype=np.int32)
    room_start[1:] = np.cumsum(sizes)
    n = int(room_start[-1])
    a = np.concatenate([np.asarray(r['points'], dtype=np.float32)[:, :6] for r in rooms]) if n else np.zeros((1, 6), np.float32)
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev), room_start, n


def _status(lib, ws, st, what):
    status = ctypes.c_int32(0)
    _lib.check(lib.lrg_edge_status(_ptr(ws), ctypes.byref(status), st), 'lrg_edge_status')
    if status.value:
        raise _lib.LrgHipError(what + ': ' + '; '.join(v for b, v in _STATUS.items() if status.value & b))


def _split(a, room_start):
    return [a[room_start[r]:room_start[r + 1]] for r in range(len(room_start) - 1)]


def _logits_device(model, pts, room_start, n, resolution, ws, st, bounds=False):
    torch = _torch()
    lib, dev = model.lib, model.device
    z = torch.empty((max(n, 1), SLOTS), dtype=torch.float64, device=dev)
    nmin = torch.empty((max(n, 1), 6), dtype=torch.float32, device=dev) if bounds else None
    nmax = torch.empty((max(n, 1), 6), dtype=torch.float32, device=dev) if bounds else None
    _lib.check(lib.lrg_edge_logits(_ptr(pts), 6, room_start.ctypes.data_as(ctypes.c_void_p), len(room_start) - 1, ctypes.c_float(resolution),
                                   _ptr(model.packed), _ptr(ws), ws.numel(), _ptr(z), _ptr(nmin), _ptr(nmax), st), 'lrg_edge_logits')
    return z, nmin, nmax


def logits(rooms, model, resolution=0.1, return_bounds=False):
    """z [n_r, 13] float64 of every room (NaN where a slot has no neighbour): the classifier's value before the logistic function,
    bit for bit the ascending-k chain of tests/edge_ref.py.  return_bounds=True adds the lists of nmin and nmax [n_r, 6] float32."""
    torch = _torch()
    dev = model.device
    if len(rooms) == 0:
        return ([], [], []) if return_bounds else []
    with torch.cuda.device(dev):
        pts, room_start, n = _batch(rooms, dev)
        ws = torch.empty(max(1, model.lib.lrg_edge_workspace_bytes(n, len(rooms), 1, 1)), dtype=torch.uint8, device=dev)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        z, nmin, nmax = _logits_device(model, pts, room_start, n, resolution, ws, st, bounds=return_bounds)
        _status(model.lib, ws, st, 'lrg_edge_logits')
        zs = _split(z[:n].cpu().numpy(), room_start)
        if return_bounds:
            return zs, _split(nmin[:n].cpu().numpy(), room_start), _split(nmax[:n].cpu().numpy(), room_start)
        return zs


def _sigmoid(model, z, sigmoid, st):
    """z (device) -> p (device) by the chosen route."""
    torch = _torch()
    if sigmoid == 'host':
        from scipy.special import expit
        return torch.from_numpy(expit(z.cpu().numpy())).to(model.device)
    p = torch.empty_like(z)
    _lib.check(model.lib.lrg_edge_sigmoid(_ptr(z), z.numel(), _ptr(p), st), 'lrg_edge_sigmoid')
    return p


def probabilities(rooms, model, resolution=0.1, sigmoid='host'):
    """p [n_r, 13] float64 of every room: ``logits`` through the logistic function by the chosen route (see ``segment``)."""
    torch = _torch()
    if sigmoid not in SIGMOID_ROUTES:
        raise ValueError('unknown sigmoid route %r (one of %s)' % (sigmoid, ', '.join(SIGMOID_ROUTES)))
    dev = model.device
    if len(rooms) == 0:
        return []
    with torch.cuda.device(dev):
        pts, room_start, n = _batch(rooms, dev)
        ws = torch.empty(max(1, model.lib.lrg_edge_workspace_bytes(n, len(rooms), 1, 1)), dtype=torch.uint8, device=dev)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        z, _, _ = _logits_device(model, pts, room_start, n, resolution, ws, st)
        _status(model.lib, ws, st, 'lrg_edge_logits')
        return _split(_sigmoid(model, z, sigmoid, st)[:n].cpu().numpy(), room_start)


def neighbour_order(q, nb_q, p_q):
    """The neighbours of q in the order the reference's search takes them (:423, :436): descending (p, b > q ? (1, b) : (0, offset)).
    nb_q [26]: the neighbour at every offset (-1: none); p_q [26]: the probability of that edge."""
    have = [o for o in range(26) if nb_q[o] >= 0]
    have.sort(key=lambda o: (p_q[o], (1, int(nb_q[o])) if nb_q[o] > q else (0, o)), reverse=True)
    return [int(nb_q[o]) for o in have]


def edge_prob(p, nb, q, o):
    """The probability of the edge from q to its neighbour at offset o: slot [q, o - 13] or [neighbour, 12 - o]."""
    return p[q, o - 13] if o >= 13 else p[nb[q, o], 12 - o]


def search(i, nb, p, cluster_label, cap=None):
    """The search of :424-436 from the unlabelled point i as a recursive DFS without duplicate pushes: the first node x != i that is
    clustered or (unlabelled and x < i).  nb [n, 26], p [n, 13] of the room, cluster_label the labels before the fallback.
    Returns (x, nodes visited); x = -1 when the component holds no such node, -2 when more than cap nodes would be visited."""
    visited = {i}
    stack = [(i, iter(neighbour_order(i, nb[i], [edge_prob(p, nb, i, o) if nb[i, o] >= 0 else 0.0 for o in range(26)])))]
    while stack:
        x = next(stack[-1][1], None)
        if x is None:
            stack.pop()
            continue
        if x in visited:
            continue
        if cluster_label[x] > 0 or x < i:
            return x, len(visited)
        if cap is not None and len(visited) >= cap:
            return -2, len(visited)
        visited.add(x)
        stack.append((x, iter(neighbour_order(x, nb[x], [edge_prob(p, nb, x, o) if nb[x, o] >= 0 else 0.0 for o in range(26)]))))
    return -1, len(visited)


def resolve(cluster_label, stop):
    """label[i] = label[stop[i]] for the searched points, in ascending i (stop[i] is clustered or smaller than i)."""
    label = np.array(cluster_label, dtype=np.int32)
    for i in np.nonzero(np.asarray(stop) >= 0)[0]:
        label[i] = label[stop[i]]
    return label


def _voxel_neighbours(points, resolution):
    """nb [n, 26] on the host (offsets in itertools.product order without the centre, -1 where the voxel is empty): one sort of the
    packed voxel keys and one binary search per offset.  For the rooms whose searches overflowed on the device."""
    import itertools
    v = np.round(points[:, :3] / np.float32(resolution)).astype(np.int64) + (1 << 20)
    pack = lambda w: (w[:, 0] << 42) | (w[:, 1] << 21) | w[:, 2]
    keys = pack(v)
    order = np.argsort(keys, kind='stable')
    ranked = keys[order]
    nb = np.full((len(points), 26), -1, dtype=np.int64)
    if len(points) == 0:
        return nb
    offsets = [x for x in itertools.product([-1, 0, 1], repeat=3) if x != (0, 0, 0)]
    for o, off in enumerate(offsets):
        want = pack(v + np.asarray(off, dtype=np.int64))
        at = np.minimum(np.searchsorted(ranked, want), len(ranked) - 1)
        hit = ranked[at] == want
        nb[hit, o] = order[at[hit]]
    return nb


def _shape_result(labels, counts, stats, return_counts, return_stats):
    """What ``segment`` returns for the flags it was given."""
    if return_counts and return_stats:
        return labels, counts, stats
    if return_counts:
        return labels, counts
    if return_stats:
        return labels, stats
    return labels


def segment(rooms, model, resolution=0.1, min_cluster_size=10, rel=0.99, floor=0.9, sigmoid='host', search_cap=1024, device=None,
            return_counts=False, return_stats=False):
    """Labels of every room in one batch (benchmarks.py --mode edge).

    rooms: list of dicts as ``baselines.room_features(raw, need_normals=False)`` returns them; model: an ``EdgeModelHIP`` (device, when
    given, must be the model's).  rel, floor: the criteria of :351-352.

    sigmoid='host' (default): the logits go to the host, through ``scipy.special.expit`` -- the function the reference's sklearn
    calls -- and back; the labels are then those of tests/edge_ref.py bit for bit.  sigmoid='device' keeps everything on the GPU; its
    probabilities can differ from expit's in the last bits.  That can change which of two edges passes a criterion only when a
    probability lies within those bits of a threshold, but saturated probabilities (1 - 1e-16, 1 - 2e-16, 1.0) are common and the
    fallback search takes a point's neighbours in the order of their probabilities: a last-bit difference can make it take another
    neighbour first, stop at another point and so give an unlabelled point another cluster's label.  Cluster counts and the labels
    of clustered points are not affected by the search.

    A search that would visit more than search_cap nodes is finished on the host by the same rule (``search``), and the labels are
    resolved again (``resolve``).  Returns a list of int32 label arrays; with return_counts also the per-room cluster counts; with
    return_stats also a dict(dead, searches, overflowed, largest_visited [whole batch], stop, cluster_labels, keep [per room]),
    None for an empty list of rooms."""
    torch = _torch()
    if sigmoid not in SIGMOID_ROUTES:
        raise ValueError('unknown sigmoid route %r (one of %s)' % (sigmoid, ', '.join(SIGMOID_ROUTES)))
    if not 1 <= min_cluster_size <= 64:
        raise ValueError('min_cluster_size must be in [1, 64]')
    if not 1 <= search_cap <= 1 << 20:
        raise ValueError('search_cap must be in [1, 2^20]')
    dev = model.device
    if device is not None and torch.device(device) != dev:
        raise ValueError('the model lives on %s, not on %s' % (dev, device))
    if len(rooms) == 0:
        return _shape_result([], np.zeros(0, np.int32), None, return_counts, return_stats)
    lib = model.lib
    with torch.cuda.device(dev):
        pts, room_start, n = _batch(rooms, dev)
        ws = torch.empty(max(1, lib.lrg_edge_workspace_bytes(n, len(rooms), min_cluster_size, search_cap)), dtype=torch.uint8, device=dev)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        z, _, _ = _logits_device(model, pts, room_start, n, resolution, ws, st)
        p = _sigmoid(model, z, sigmoid, st)
        labels, counts, stats = _segment_device(rooms, p, model, pts, room_start, n, ws, st, True, resolution, min_cluster_size, rel, floor,
                                                search_cap)
    return _shape_result(labels, counts, stats, return_counts, return_stats)


def segment_probabilities(rooms, p, model, resolution=0.1, min_cluster_size=10, rel=0.99, floor=0.9, search_cap=1024):
    """The stages after the logistic function (``lrg_edge_segment``) on given probabilities: p is a list of [n_r, 13] float64 arrays.
    Returns (labels, counts, stats) as ``segment`` describes them."""
    torch = _torch()
    lib, dev = model.lib, model.device
    with torch.cuda.device(dev):
        pts, room_start, n = _batch(rooms, dev)
        ws = torch.empty(max(1, lib.lrg_edge_workspace_bytes(n, len(rooms), min_cluster_size, search_cap)), dtype=torch.uint8, device=dev)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        cat = np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1, SLOTS) for x in p]) if n else np.zeros((1, SLOTS))
        if len(cat) != max(n, 1):
            raise ValueError('p has %d rows, the rooms %d points' % (len(cat), n))
        pd = torch.from_numpy(np.ascontiguousarray(cat)).to(dev)
        return _segment_device(rooms, pd, model, pts, room_start, n, ws, st, False, resolution, min_cluster_size, rel, floor, search_cap)


def _segment_device(rooms, p, model, pts, room_start, n, ws, st, prepared, resolution, min_cluster_size, rel, floor, search_cap):
    """``lrg_edge_segment`` on the batch (pts, room_start) with p [n, 13] on the device, then the host's share.  prepared: ws is the
    workspace ``lrg_edge_logits`` has just run on for this batch, so its hash and neighbour table are not built again."""
    torch = _torch()
    lib, dev = model.lib, model.device
    labels = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    stop = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    clab = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    keep = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    counts = torch.empty(len(rooms), dtype=torch.int32, device=dev)
    counters = torch.zeros(4, dtype=torch.int32, device=dev)
    _lib.check(lib.lrg_edge_segment(_ptr(pts), 6, room_start.ctypes.data_as(ctypes.c_void_p), len(rooms), ctypes.c_float(resolution), _ptr(p),
                                    float(rel), float(floor), min_cluster_size, search_cap, _ptr(ws), ws.numel(), _ptr(labels), _ptr(counts),
                                    _ptr(stop), _ptr(counters), _ptr(keep), _ptr(clab), 1 if prepared else 0, st), 'lrg_edge_segment')
    _status(lib, ws, st, 'lrg_edge_segment')
    dead, searches, overflowed, largest = (int(x) for x in counters.cpu().numpy())
    lab = labels[:n].cpu().numpy()
    stop_h = stop[:n].cpu().numpy()
    clab_h = clab[:n].cpu().numpy()
    keep_h = keep[:n].cpu().numpy().view(np.uint32)
    out = _split(lab, room_start)
    stops = [np.where(s >= 0, s - room_start[r], s).astype(np.int32) for r, s in enumerate(_split(stop_h, room_start))]   # batch index -> the room's
    if overflowed:                                                  # finished on the host by the same rule, then resolved again
        p_h = p[:n].cpu().numpy()
        for r, room in enumerate(rooms):
            if not (stops[r] == -2).any():
                continue
            s, e = int(room_start[r]), int(room_start[r + 1])
            nb = _voxel_neighbours(np.asarray(room['points'], dtype=np.float32), resolution)
            for i in np.nonzero(stops[r] == -2)[0]:
                stops[r][i], visited = search(int(i), nb, p_h[s:e], clab_h[s:e])
                largest = max(largest, visited)
            out[r] = resolve(clab_h[s:e], stops[r])
    stats = dict(dead=dead, searches=searches, overflowed=overflowed, largest_visited=largest, stop=stops,
                 cluster_labels=_split(clab_h, room_start), keep=_split(keep_h, room_start))
    return out, counts.cpu().numpy(), stats


def components(rooms, keep, model, resolution=0.1, min_cluster_size=10):
    """``lrg_baseline_segment_mask`` on its own: the clusters of given keep words (a list of [n_r] uint32 arrays)."""
    torch = _torch()
    lib, dev = model.lib, model.device
    with torch.cuda.device(dev):
        pts, room_start, n = _batch(rooms, dev)
        kw = np.concatenate([np.asarray(k, dtype=np.uint32) for k in keep]) if n else np.zeros(1, np.uint32)
        kd = torch.from_numpy(kw.view(np.int32).copy()).to(dev)
        ws = torch.empty(max(1, lib.lrg_baseline_workspace_bytes(n, len(rooms), min_cluster_size)), dtype=torch.uint8, device=dev)
        labels = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        counts = torch.empty(len(rooms), dtype=torch.int32, device=dev)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.lrg_baseline_segment_mask(_ptr(pts), 6, room_start.ctypes.data_as(ctypes.c_void_p), len(rooms), ctypes.c_float(resolution),
                                                 _ptr(kd), min_cluster_size, _ptr(ws), ws.numel(), _ptr(labels), _ptr(counts), st),
                   'lrg_baseline_segment_mask')
        from . import baselines
        return baselines._finish(lib, ws, st, n, rooms, room_start, min_cluster_size, labels, counts, True, False, None,
                                 'lrg_baseline_segment_mask')
