"""MCPNet, the learned baseline of the reference's test_mcpnet.py (network: learn_region_grow_util.py:191-225), on the GPU.

``prepare_room``  test_mcpnet.py:71-92 for one room: centring on the host in float32, then the device equalisation of
                  ``baselines.room_features`` (first point per 0.1 m voxel).  Centring comes first here, unlike test_region_grow.py.
``neighbors``     :95-107 for a batch of rooms: candidate lists on 0.3 m cells (``lrg_mcp_candidates``) and 50 neighbour rows per
                  point (``lrg_mcp_neighbors``).  rng='legacy' draws ``numpy.random.choice(count, 50, replace=count < 50)`` on the
                  host from one RandomState in room order (the reference's stream; pass ``state`` to carry it across calls);
                  rng='counter' draws on the device from Philox keyed by (seed, room id).
``MCPNetHIP``     the network: ``embed(points, nbr)`` -> [n, 10] float32 in one launch (``lrg_mcp_embed``).
``segment``       :122-145 for a batch of rooms: edges where emb[k].dot(emb[i]) > threshold on the 26-neighbour voxel graph and
                  the components of more than min_cluster_size points (``lrg_baseline_segment_embedding``).

There is no CPU fallback: without the library or a GPU, ``_lib.LrgHipError`` is raised.  DESIGN.md §3.9.
"""
import ctypes

import numpy as np
import torch

from . import _lib, baselines
from .checkpoint import MCPNET_SHAPES

NUM_NEIGHBORS = 50           # test_mcpnet.py:19
NEIGHBOR_RADIUS = 0.3        # :20
RESOLUTION = 0.1             # :17
EMBEDDING_SIZE = 10          # :22
RNG_MODES = ('legacy', 'counter')
_STATUS = {1: 'a point lies outside the +-2^20 cell window', 2: 'a legacy position lies outside [0, candidate count)'}


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _device(device):
    if not torch.cuda.is_available():
        raise _lib.LrgHipError('learn_region_grow_amd.mcpnet needs a GPU (there is no CPU fallback)')
    return torch.device(device if device is not None else 'cuda:0')


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def center_room(unequalized_points):
    """test_mcpnet.py:71-73 in float32: x and y minus the centre of their range, z minus its minimum.  Returns a copy [M, 6]."""
    p = np.array(np.asarray(unequalized_points)[:, :6], dtype=np.float32)
    centroid = 0.5 * (p[:, :2].min(axis=0) + p[:, :2].max(axis=0))
    p[:, :2] -= centroid
    p[:, 2] -= p[:, 2].min()
    return p


def prepare_room(unequalized_points, room_id=0, device=None):
    """dict(points [N, 6] float32 centred and equalised, centred [M, 6] every raw point centred, equalized_idx, unequalized_idx,
    room_id).  room_id keys the counter RNG."""
    centred = center_room(unequalized_points)
    f = baselines.room_features(centred, resolution=RESOLUTION, need_normals=False, device=device)
    return dict(points=f['points'], centred=centred, equalized_idx=f['equalized_idx'], unequalized_idx=f['unequalized_idx'],
                room_id=int(room_id))


def _batch(rooms, dev):
    sizes = [len(r['points']) for r in rooms]
    room_start = np.zeros(len(rooms) + 1, dtype=np.int32)
    room_start[1:] = np.cumsum(sizes)
    n = int(room_start[-1])
    pts = np.concatenate([np.asarray(r['points'], dtype=np.float32).reshape(-1, 6) for r in rooms]) if n else np.zeros((1, 6), np.float32)
    return room_start, n, torch.from_numpy(np.ascontiguousarray(pts)).to(dev)


def legacy_positions(counts, state):
    """Positions into each point's candidate list, drawn as test_mcpnet.py:104 draws them: choice(count, 50, replace=count < 50) per
    point in order, from the RandomState `state` (numpy.random.choice(list) consumes and returns what choice(len(list)) does)."""
    out = np.empty((len(counts), NUM_NEIGHBORS), dtype=np.int32)
    for i, c in enumerate(np.asarray(counts).tolist()):
        out[i] = state.choice(c, NUM_NEIGHBORS, replace=c < NUM_NEIGHBORS)
    return out


def neighbors(rooms, rng='legacy', seed=0, state=None, device=None, return_counts=False):
    """[n_r, 50] int32 neighbour indices (into each room's own points) for every room of the batch, in one candidate build.

    rooms: dicts with 'points' (centred, equalised: prepare_room) and, for rng='counter', 'room_id' (default: position in the list).
    rng='legacy': `state` (a numpy RandomState; default RandomState(seed)) is advanced in room order, point order.
    Returns the list (and the per-room candidate counts with return_counts=True)."""
    if rng not in RNG_MODES:
        raise ValueError('rng must be one of %s' % (RNG_MODES,))
    if len(rooms) == 0:
        return ([], []) if return_counts else []
    lib = _lib.load()
    dev = _device(device)
    with torch.cuda.device(dev):
        room_start, n, pts = _batch(rooms, dev)
        ws = torch.empty(max(1, lib.lrg_mcp_workspace_bytes(n, len(rooms))), dtype=torch.uint8, device=dev)
        counts = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        nbr = torch.empty((max(n, 1), NUM_NEIGHBORS), dtype=torch.int32, device=dev)
        st = _stream()
        rs_p = room_start.ctypes.data_as(ctypes.c_void_p)
        _lib.check(lib.lrg_mcp_candidates(_ptr(pts), 6, rs_p, len(rooms), _ptr(ws), ws.numel(), _ptr(counts), st), 'lrg_mcp_candidates')
        status = ctypes.c_int32(0)
        _lib.check(lib.lrg_mcp_status(_ptr(ws), n, len(rooms), ctypes.byref(status), st), 'lrg_mcp_status')
        if status.value:
            raise _lib.LrgHipError('lrg_mcp_candidates: ' + '; '.join(v for b, v in _STATUS.items() if status.value & b))
        cnt = counts[:n].cpu().numpy()
        if rng == 'legacy':
            if state is None:
                state = np.random.RandomState(seed)
            pos = torch.from_numpy(legacy_positions(cnt, state)).to(dev) if n else nbr
            _lib.check(lib.lrg_mcp_neighbors(_ptr(pts), 6, rs_p, len(rooms), _ptr(ws), ws.numel(), _ptr(pos), 0, None, _ptr(nbr), st),
                       'lrg_mcp_neighbors')
        else:
            ids = np.array([int(r.get('room_id', k)) for k, r in enumerate(rooms)], dtype=np.int32)
            _lib.check(lib.lrg_mcp_neighbors(_ptr(pts), 6, rs_p, len(rooms), _ptr(ws), ws.numel(), None, ctypes.c_uint32(int(seed) & 0xFFFFFFFF),
                                             ids.ctypes.data_as(ctypes.c_void_p), _ptr(nbr), st), 'lrg_mcp_neighbors')
        _lib.check(lib.lrg_mcp_status(_ptr(ws), n, len(rooms), ctypes.byref(status), st), 'lrg_mcp_status')
        if status.value:
            raise _lib.LrgHipError('lrg_mcp_neighbors: ' + '; '.join(v for b, v in _STATUS.items() if status.value & b))
        out = nbr[:n].cpu().numpy()
    res = [out[room_start[r]:room_start[r + 1]] - room_start[r] for r in range(len(rooms))]
    cnts = [cnt[room_start[r]:room_start[r + 1]] for r in range(len(rooms))]
    return (res, cnts) if return_counts else res


class MCPNetHIP:
    """MCPNet's embedding network (learn_region_grow_util.py:210-225) on gfx950.  weights: name -> array of the eight mcp_*
    trainables in their TF shapes (checkpoint.load_mcpnet_weights)."""

    def __init__(self, weights, device=None):
        self.lib = _lib.load()
        self.device = _device(device)
        for k, shp in MCPNET_SHAPES.items():
            if k not in weights:
                raise KeyError('MCPNet weight %s missing' % k)
            if tuple(np.shape(weights[k])) != shp:
                raise ValueError('%s has shape %s, MCPNet needs %s' % (k, np.shape(weights[k]), shp))
        with torch.cuda.device(self.device):
            w = {k: torch.from_numpy(np.ascontiguousarray(weights[k], dtype=np.float32)).to(self.device) for k in MCPNET_SHAPES}
            self.packed = torch.empty(self.lib.lrg_mcp_packed_floats(), dtype=torch.float32, device=self.device)
            _lib.check(self.lib.lrg_mcp_pack_weights(*[_ptr(w[k]) for k in ('mcp_kernel1', 'mcp_bias1', 'mcp_kernel2', 'mcp_bias2',
                                                                          'mcp_kernel3', 'mcp_bias3', 'mcp_kernel4', 'mcp_bias4')],
                                                     _ptr(self.packed), _stream()), 'lrg_mcp_pack_weights')
            torch.cuda.current_stream().synchronize()

    def embed_device(self, pts, nbr, out=None, status=None):
        """Device tensors: pts [n, ld >= 6] float32, nbr [n, 50] int32 (indices into pts) -> [n, 10] float32 (no synchronisation;
        status: an int32 device word that gets bit 1 for an out-of-range index)."""
        n = pts.shape[0]
        if out is None:
            out = torch.empty((max(n, 1), EMBEDDING_SIZE), dtype=torch.float32, device=pts.device)
        if status is None:
            status = torch.zeros(1, dtype=torch.int32, device=pts.device)
        _lib.check(self.lib.lrg_mcp_embed(_ptr(pts), pts.stride(0), n, _ptr(nbr), _ptr(self.packed), _ptr(out), _ptr(status), _stream()),
                   'lrg_mcp_embed')
        return out[:n]

    def embed(self, points, nbr):
        """points [n, >= 6] (a room, or a list of rooms), nbr [n, 50] indices into the same room -> float32 [n, 10] (a list for a list)."""
        single = not isinstance(points, (list, tuple))
        plist = [points] if single else list(points)
        nlist = [nbr] if single else list(nbr)
        sizes = [len(p) for p in plist]
        start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        n = int(start[-1])
        if n == 0:
            out = [np.zeros((0, EMBEDDING_SIZE), np.float32) for _ in plist]
            return out[0] if single else out
        p = np.concatenate([np.asarray(x, dtype=np.float32)[:, :6] for x in plist])
        q = np.concatenate([np.asarray(y, dtype=np.int64).reshape(-1, NUM_NEIGHBORS) + start[k] for k, y in enumerate(nlist)])
        with torch.cuda.device(self.device):
            pts = torch.from_numpy(np.ascontiguousarray(p)).to(self.device)
            nb = torch.from_numpy(q.astype(np.int32)).to(self.device)
            status = torch.zeros(1, dtype=torch.int32, device=self.device)
            emb = self.embed_device(pts, nb, status=status).cpu().numpy()
            if int(status.item()):
                raise _lib.LrgHipError('lrg_mcp_embed: a neighbour index lies outside its room')
        out = [emb[start[k]:start[k + 1]] for k in range(len(plist))]
        return out[0] if single else out


def segment(rooms, embeddings, threshold=0.9, min_cluster_size=10, device=None, return_counts=False):
    """cluster_label of every room (test_mcpnet.py:122-145) in ONE lrg_baseline_segment_embedding call.  rooms: dicts with 'points'
    (equalised); embeddings: one [n_r, dim] array per room.  Returns int32 label arrays (0 = no cluster)."""
    if len(rooms) != len(embeddings):
        raise ValueError('one embedding array per room')
    if not 1 <= min_cluster_size <= baselines.MAX_MIN_CLUSTER_SIZE:
        raise ValueError('min_cluster_size must be in [1, %d]' % baselines.MAX_MIN_CLUSTER_SIZE)
    if len(rooms) == 0:
        return ([], np.zeros(0, np.int32)) if return_counts else []
    lib = _lib.load()
    dev = _device(device)
    dim = int(np.shape(embeddings[0])[1]) if np.ndim(embeddings[0]) == 2 else EMBEDDING_SIZE
    for r, e in zip(rooms, embeddings):
        if np.shape(e) != (len(r['points']), dim):
            raise ValueError('embeddings must be [n_points, %d] per room' % dim)
    with torch.cuda.device(dev):
        room_start, n, pts = _batch(rooms, dev)
        e = np.concatenate([np.asarray(x, dtype=np.float32) for x in embeddings]) if n else np.zeros((1, dim), np.float32)
        emb = torch.from_numpy(np.ascontiguousarray(e)).to(dev)
        ws = torch.empty(max(1, lib.lrg_baseline_workspace_bytes(n, len(rooms), min_cluster_size)), dtype=torch.uint8, device=dev)
        labels = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        counts = torch.empty(len(rooms), dtype=torch.int32, device=dev)
        st = _stream()
        _lib.check(lib.lrg_baseline_segment_embedding(_ptr(pts), 6, room_start.ctypes.data_as(ctypes.c_void_p), len(rooms),
                                                      ctypes.c_float(RESOLUTION), _ptr(emb), dim, float(threshold), min_cluster_size,
                                                      _ptr(ws), ws.numel(), _ptr(labels), _ptr(counts), st), 'lrg_baseline_segment_embedding')
        status = ctypes.c_int32(0)
        _lib.check(lib.lrg_baseline_status(_ptr(ws), n, len(rooms), min_cluster_size, ctypes.byref(status), st), 'lrg_baseline_status')
        if status.value:
            raise _lib.LrgHipError('lrg_baseline_segment_embedding: status %d (1: voxel window, 2: the room is not equalised)' % status.value)
        lab = labels[:n].cpu().numpy()
        cnt = counts.cpu().numpy()
    out = [lab[room_start[r]:room_start[r + 1]] for r in range(len(rooms))]
    return (out, cnt) if return_counts else out


def embedding_colors(embeddings):
    """test_mcpnet.py:186-187: a 3-component sklearn PCA of the embeddings (float64), min-max scaled to 0 .. 255 per component."""
    from sklearn.decomposition import PCA
    x = PCA(n_components=3).fit_transform(np.asarray(embeddings, dtype=np.float64))
    return (x - x.min(axis=0)) / (x.max(axis=0) - x.min(axis=0)) * 255


def result_colors(cluster_label2):
    """test_mcpnet.py:190-191: RandomState(0).randint(0, 255, (max + 1, 3))[cluster_label2]."""
    c = np.asarray(cluster_label2)
    return np.random.RandomState(0).randint(0, 255, (int(np.max(c)) + 1, 3))[c, :]
