"""PointNet2, the learned baseline of the reference's ``benchmarks.py --mode pointnet2`` (network: train_pointnet.py:113-202), on
the GPU.

``prepare_room``   benchmarks.py:199-215 for one room: the device equalisation of ``baselines.room_features`` (first point per
                   0.1 m voxel); no normals.
``cells``          :283-287: the xy cells of a room's equalised points, round(xy / grid_resolution) in float32, half to even; every
                   cell's point indices in ascending order.  Host code: one stable sort by cell key.
``cell_inputs``    :288-295: the [B, 1024, 6] float32 network inputs -- x and y minus the cell centre, z minus the cell's minimum,
                   rows beyond the cell's count copies of its first row (they take part in the sampling and the ball queries, so
                   they are reproduced, not masked).  A cell of more than 1024 points makes the reference fail at :298; here it is
                   a ValueError naming the room and the cell.
``PointNet2HIP``   the network.  ``logits(batch)`` -> [B, 1024, num_class]; ``classify(rooms, area=...)`` -> per-room int32 classes
                   (:296-298).
``segment``        :300-306 and :405-416 for a batch of rooms: edges between 26-neighbour voxels of equal class and the components
                   of more than min_cluster_size points (``lrg_baseline_segment_labels``).

There is no CPU fallback: without the library or a GPU, ``_lib.LrgHipError`` is raised.  DESIGN.md §3.11.
"""
import ctypes

import numpy as np
import torch

from . import _lib, baselines
from .checkpoint import POINTNET2_FP_MLPS, POINTNET2_SA_MLPS, pointnet2_variable_shapes, pointnet2_variant, BundleError

NUM_POINT = 1024             # benchmarks.py:30
NSAMPLE = 32                 # train_pointnet.py:181-184
RESOLUTION = 0.1             # benchmarks.py:119
SA_LEVELS = ((1024, 0.1), (256, 0.2), (64, 0.4), (16, 0.8))        # (npoint, radius), train_pointnet.py:181-184
CHUNK_CELLS = 64             # cells per pass through the network (PointNet2HIP.logits)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _device(device):
    if not torch.cuda.is_available():
        raise _lib.LrgHipError('learn_region_grow_amd.pointnet2 needs a GPU (there is no CPU fallback)')
    return torch.device(device if device is not None else 'cuda:0')


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def grid_resolution(area):
    """benchmarks.py:283: 3.0 if the area's name contains 'kitti', else 1.0."""
    return 3.0 if 'kitti' in str(area) else 1.0


def prepare_room(unequalized_points, device=None):
    """dict(points [N, 6] float32 equalised, equalized_idx, unequalized_idx) (benchmarks.py:199-215)."""
    f = baselines.room_features(unequalized_points, resolution=RESOLUTION, need_normals=False, device=device)
    return dict(points=f['points'], equalized_idx=f['equalized_idx'], unequalized_idx=f['unequalized_idx'])


def cells(points, grid_resolution):
    """-> (keys [C, 2] int64, members: C int64 arrays of point indices in ascending order).  The cell of a point is
    numpy.round(points[:, :2] / grid_resolution).astype(int) on float32 (benchmarks.py:284).  Cells come sorted by key; nothing
    depends on their order."""
    p = np.asarray(points, dtype=np.float32)
    grid = np.round(p[:, :2] / np.float32(grid_resolution)).astype(np.int64)
    if len(grid) == 0:
        return np.zeros((0, 2), np.int64), []
    keys, inverse = np.unique(grid, axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    order = np.argsort(inverse, kind='stable')                       # by cell, ascending index inside a cell
    bounds = np.concatenate([[0], np.cumsum(np.bincount(inverse, minlength=len(keys)))])
    return keys, [order[bounds[c]:bounds[c + 1]] for c in range(len(keys))]


def cell_inputs(points, grid_resolution, room=None):
    """-> (batch [C, 1024, 6] float32, members, keys) for one room's equalised points: benchmarks.py:288-295.  members[c] maps the
    first len(members[c]) rows of batch[c] back to point indices.  room: what the ValueError calls the room."""
    p = np.asarray(points, dtype=np.float32)[:, :6]
    keys, members = cells(p, grid_resolution)
    batch = np.empty((len(keys), NUM_POINT, 6), dtype=np.float32)
    for c, idx in enumerate(members):
        if len(idx) > NUM_POINT:
            raise ValueError('room %s: cell (%d, %d) holds %d points, more than the network\'s %d (benchmarks.py:298 fails there too)'
                             % (room if room is not None else '?', keys[c][0], keys[c][1], len(idx), NUM_POINT))
        rows = p[idx].copy()
        rows[:, :2] -= (keys[c] * float(grid_resolution)).astype(np.float32)      # numpy.array(g) * grid_resolution: exact in float32
        rows[:, 2] -= rows[:, 2].min()
        batch[c, :len(idx)] = rows
        batch[c, len(idx):] = rows[0]
    return batch, members, keys


class PointNet2HIP:
    """PointNet2 (train_pointnet.py:170-202) on gfx950.  weights: name -> array of the 46 trainables in their TF shapes
    (checkpoint.load_pointnet2_weights).  The variant (colour features or not) and the class count are read from the shapes."""

    def __init__(self, weights, device=None):
        self.lib = _lib.load()
        self.device = _device(device)
        try:
            self.num_class, self.rgb_features = pointnet2_variant({k: np.shape(v) for k, v in weights.items()})
        except BundleError as e:
            raise ValueError(str(e))
        for k, shp in pointnet2_variable_shapes(self.num_class, self.rgb_features).items():
            if k not in weights:
                raise KeyError('PointNet2 weight %s missing' % k)
            if tuple(np.shape(weights[k])) != tuple(shp):
                raise ValueError('%s has shape %s, PointNet2 needs %s' % (k, np.shape(weights[k]), shp))
        with torch.cuda.device(self.device):
            self.sa = [self._pack(weights, 'layer%d/' % (lv + 1), range(len(m))) for lv, m in enumerate(POINTNET2_SA_MLPS)]
            self.fp = [self._pack(weights, 'fa_layer%d/' % (lv + 1), range(len(m))) for lv, m in enumerate(POINTNET2_FP_MLPS)]
            self.head = self._pack(weights, '', (1, 2))
            torch.cuda.current_stream().synchronize()

    def _pack(self, weights, scope, ids):
        """-> (packed device tensor, widths int32 array of the layers' outputs, input width)"""
        layers = []
        for i in ids:
            w = np.ascontiguousarray(weights['%skernel%d' % (scope, i)], dtype=np.float32)
            layers.append((w.reshape(w.shape[-2], w.shape[-1]), np.ascontiguousarray(weights['%sbias%d' % (scope, i)], dtype=np.float32)))
        sizes = [self.lib.lrg_pointnet2_packed_floats(w.shape[0], w.shape[1]) for w, _ in layers]
        packed = torch.empty(sum(sizes), dtype=torch.float32, device=self.device)
        off = 0
        for (w, b), size in zip(layers, sizes):
            wd, bd = torch.from_numpy(w).to(self.device), torch.from_numpy(b).to(self.device)
            _lib.check(self.lib.lrg_pointnet2_pack_layer(w.shape[0], w.shape[1], _ptr(wd), _ptr(bd), _ptr(packed[off:]), _stream()),
                       'lrg_pointnet2_pack_layer')
            off += size
        torch.cuda.current_stream().synchronize()                    # wd, bd may go
        return packed, np.array([w.shape[1] for w, _ in layers], dtype=np.int32), layers[0][0].shape[0]

    def _group_mlp(self, xyz, new_xyz, points, idx, mlp):
        packed, widths, cin = mlp
        b, n, _ = xyz.shape
        m = new_xyz.shape[1]
        c = 0 if points is None else points.shape[2]
        if 3 + c != cin:
            raise ValueError('the level reads %d channels, its kernel0 has %d' % (3 + c, cin))
        out = torch.empty((b, m, int(widths[-1])), dtype=torch.float32, device=xyz.device)
        _lib.check(self.lib.lrg_pointnet2_group_mlp(b, n, m, NSAMPLE, c, _ptr(xyz), _ptr(new_xyz), _ptr(points), _ptr(idx),
                                                    widths.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _ptr(packed), _ptr(out), _stream()),
                   'lrg_pointnet2_group_mlp')
        return out

    def _row_mlp(self, a, b, mlp, relu_last=True):
        packed, widths, cin = mlp
        r = a.shape[0] * a.shape[1]
        ca, cb = a.shape[2], 0 if b is None else b.shape[2]
        if ca + cb != cin:
            raise ValueError('the level reads %d channels, its first kernel has %d' % (ca + cb, cin))
        out = torch.empty((a.shape[0], a.shape[1], int(widths[-1])), dtype=torch.float32, device=a.device)
        _lib.check(self.lib.lrg_pointnet2_row_mlp(r, ca, cb, _ptr(a), _ptr(b), len(widths), widths.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                  1 if relu_last else 0, _ptr(packed), _ptr(out), _stream()), 'lrg_pointnet2_row_mlp')
        return out

    def _forward(self, x, levels=None, mark=None):
        """x [b, 1024, 6] float32 on the device -> logits [b, 1024, num_class].  25 launches, whatever b is: per set-abstraction
        level lrg_farthest_point_sample, lrg_gather_point, lrg_query_ball_point, lrg_pointnet2_group_mlp; per feature-propagation
        level lrg_three_nn_interpolate, lrg_pointnet2_row_mlp; the head is one lrg_pointnet2_row_mlp of two layers.  mark(name), if
        given, is called after every launch (tools/pointnet2_bench.py records an event there)."""
        from . import grouping, sampling
        mark = mark or (lambda name: None)
        b = x.shape[0]
        xyz = [x[:, :, :3].contiguous()]
        feat = [x[:, :, 3:].contiguous() if self.rgb_features else None]
        for lv, (npoint, radius) in enumerate(SA_LEVELS):
            fps = sampling.farthest_point_sample(npoint, xyz[lv])
            mark('fps')
            new_xyz = sampling.gather_point(xyz[lv], fps)
            mark('gather')
            idx, _ = grouping.query_ball_point(radius, NSAMPLE, xyz[lv], new_xyz)
            mark('ball_query')
            new_feat = self._group_mlp(xyz[lv], new_xyz, feat[lv], idx, self.sa[lv])
            mark('group_mlp')
            xyz.append(new_xyz)
            feat.append(new_feat)
            if levels is not None:
                levels['sa'].append(dict(fps=fps, new_xyz=new_xyz, idx=idx, features=new_feat))
        up = feat[4]
        for lv in range(4):                                           # fa_layer1: l4 -> l3, ..., fa_layer4: l1 -> l0
            dst = 3 - lv
            n, m, c = xyz[dst].shape[1], xyz[dst + 1].shape[1], up.shape[2]
            interp = torch.empty((b, n, c), dtype=torch.float32, device=x.device)
            nn_idx = torch.empty((b, n, 3), dtype=torch.int32, device=x.device) if levels is not None else None
            _lib.check(self.lib.lrg_three_nn_interpolate(b, n, m, c, _ptr(xyz[dst]), _ptr(xyz[dst + 1]), _ptr(up), None, _ptr(nn_idx), None,
                                                         _ptr(interp), _stream()), 'lrg_three_nn_interpolate')
            mark('three_nn_interpolate')
            up = self._row_mlp(interp, feat[dst], self.fp[lv])
            mark('row_mlp')
            if levels is not None:
                levels['fp'].append(dict(nn_idx=nn_idx, interpolated=interp, features=up))
        out = self._row_mlp(up, None, self.head, relu_last=False)
        mark('head')
        return out

    def logits(self, batch, return_levels=False):
        """batch [B, 1024, 6] float32 (cell_inputs) -> float32 [B, 1024, num_class]; all cells go through the network together, each
        level a fixed number of launches.  With return_levels also dict(sa=[4 x dict(fps, new_xyz, idx, features)],
        fp=[4 x dict(nn_idx, interpolated, features)]) of NumPy arrays.

        More than CHUNK_CELLS = 64 cells are processed 64 at a time.  Per cell the pass holds, in floats or int32: the input 6 K
        (K = 1024), the levels' xyz 4 K, the ball-query indices 32 (1024 + 256 + 64 + 16) = 42.5 K, the levels' features
        64 K + 32 K + 16 K + 8 K = 120 K, the interpolated rows 32 K + 64 K + 256 K + 128 K = 480 K, the propagated features
        16 K + 64 K + 128 K + 128 K = 336 K and the logits num_class K (260 K for kitti): 1.25 M words = 5 MB, so a pass of 64
        cells stays under 330 MB however many cells the call has.  Every op works on one batch element (cell) at a time, so the
        result does not depend on the chunking."""
        batch = np.ascontiguousarray(batch, dtype=np.float32)
        if batch.ndim != 3 or batch.shape[1:] != (NUM_POINT, 6):
            raise ValueError('batch must be [B, %d, 6]' % NUM_POINT)
        out = np.empty((len(batch), NUM_POINT, self.num_class), dtype=np.float32)
        all_levels = []
        with torch.cuda.device(self.device):
            for c0 in range(0, len(batch), CHUNK_CELLS):
                x = torch.from_numpy(batch[c0:c0 + CHUNK_CELLS]).to(self.device)
                lv = dict(sa=[], fp=[]) if return_levels else None
                out[c0:c0 + CHUNK_CELLS] = self._forward(x, lv).cpu().numpy()
                if return_levels:
                    all_levels.append(lv)
        if not return_levels:
            return out
        merged = dict(sa=[], fp=[])
        for kind in ('sa', 'fp'):
            for lv in range(4):
                names = all_levels[0][kind][lv].keys() if all_levels else ()
                merged[kind].append({k: np.concatenate([ch[kind][lv][k].cpu().numpy() for ch in all_levels]) for k in names})
        return out, merged

    def classify_cells(self, batch):
        """batch [B, 1024, 6] -> int32 [B, 1024]: the argmax of every row's logits on the device, a tie to the lowest class as
        numpy.argmax (benchmarks.py:297)."""
        return classify_cells(self, batch, CHUNK_CELLS)

    def classify(self, rooms, area=None, grid_resolution_m=None):
        """class_labels of every room (benchmarks.py:282-298): rooms are dicts with 'points' (equalised: prepare_room) or [N, >= 6]
        arrays.  The cells of ALL rooms go through the network together.  area picks the cell size as :283 does (or give
        grid_resolution_m).  Returns one int32 array per room."""
        return classify_rooms(self, rooms, area, grid_resolution_m)


def classify_cells(net, batch, chunk_cells):
    """PointNet2HIP.classify_cells and PointNetHIP.classify_cells: net._forward(x) -> logits [b, 1024, net.num_class] on
    net.device, chunk_cells cells at a time."""
    batch = np.ascontiguousarray(batch, dtype=np.float32)
    out = np.empty((len(batch), NUM_POINT), dtype=np.int32)
    with torch.cuda.device(net.device):
        classes = torch.arange(net.num_class, dtype=torch.int32, device=net.device)
        for c0 in range(0, len(batch), chunk_cells):
            lg = net._forward(torch.from_numpy(batch[c0:c0 + chunk_cells]).to(net.device))
            best = lg.amax(dim=2, keepdim=True)
            first = torch.where(lg == best, classes, net.num_class).amin(dim=2)         # the lowest index among equal maxima
            out[c0:c0 + chunk_cells] = first.to(torch.int32).cpu().numpy()
    return out


def classify_rooms(net, rooms, area=None, grid_resolution_m=None):
    """PointNet2HIP.classify and PointNetHIP.classify: the cells of all rooms through net.classify_cells together."""
    res = float(grid_resolution_m) if grid_resolution_m is not None else grid_resolution(area)
    pts = [np.asarray(r['points'] if isinstance(r, dict) else r, dtype=np.float32) for r in rooms]
    batches, maps = [], []
    for k, p in enumerate(pts):
        name = rooms[k].get('room_id', k) if isinstance(rooms[k], dict) else k
        batch, members, _ = cell_inputs(p, res, room=name)
        batches.append(batch)
        maps.append(members)
    out = [np.zeros(len(p), dtype=np.int32) for p in pts]
    if not batches or sum(len(b) for b in batches) == 0:
        return out
    cls = net.classify_cells(np.concatenate(batches))
    c = 0
    for k, members in enumerate(maps):
        for idx in members:
            out[k][idx] = cls[c, :len(idx)]
            c += 1
    return out


def segment(rooms, classes, min_cluster_size=10, device=None, return_counts=False):
    """cluster_label of every room (benchmarks.py:300-306, :405-416) in ONE lrg_baseline_segment_labels call.  rooms: dicts with
    'points' (equalised); classes: one integer array [n_r] per room.  Returns int32 label arrays (0 = no cluster)."""
    if len(rooms) != len(classes):
        raise ValueError('one class array per room')
    if not 1 <= min_cluster_size <= baselines.MAX_MIN_CLUSTER_SIZE:
        raise ValueError('min_cluster_size must be in [1, %d]' % baselines.MAX_MIN_CLUSTER_SIZE)
    if len(rooms) == 0:
        return ([], np.zeros(0, np.int32)) if return_counts else []
    for r, c in zip(rooms, classes):
        if np.shape(c) != (len(r['points']),):
            raise ValueError('classes must be [n_points] per room')
    lib = _lib.load()
    dev = _device(device)
    sizes = [len(r['points']) for r in rooms]
    room_start = np.zeros(len(rooms) + 1, dtype=np.int32)
    room_start[1:] = np.cumsum(sizes)
    n = int(room_start[-1])
    p = np.concatenate([np.asarray(r['points'], dtype=np.float32).reshape(-1, 6) for r in rooms]) if n else np.zeros((1, 6), np.float32)
    c = np.concatenate([np.asarray(x).astype(np.int32) for x in classes]) if n else np.zeros(1, np.int32)
    with torch.cuda.device(dev):
        pts = torch.from_numpy(np.ascontiguousarray(p)).to(dev)
        cls = torch.from_numpy(np.ascontiguousarray(c)).to(dev)
        ws = torch.empty(max(1, lib.lrg_baseline_workspace_bytes(n, len(rooms), min_cluster_size)), dtype=torch.uint8, device=dev)
        labels = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        counts = torch.empty(len(rooms), dtype=torch.int32, device=dev)
        st = _stream()
        _lib.check(lib.lrg_baseline_segment_labels(_ptr(pts), 6, room_start.ctypes.data_as(ctypes.c_void_p), len(rooms), ctypes.c_float(RESOLUTION),
                                                   _ptr(cls), min_cluster_size, _ptr(ws), ws.numel(), _ptr(labels), _ptr(counts), st),
                   'lrg_baseline_segment_labels')
        status = ctypes.c_int32(0)
        _lib.check(lib.lrg_baseline_status(_ptr(ws), n, len(rooms), min_cluster_size, ctypes.byref(status), st), 'lrg_baseline_status')
        if status.value:
            raise _lib.LrgHipError('lrg_baseline_segment_labels: status %d (1: voxel window, 2: the room is not equalised)' % status.value)
        lab = labels[:n].cpu().numpy()
        cnt = counts.cpu().numpy()
    out = [lab[room_start[r]:room_start[r + 1]] for r in range(len(rooms))]
    return (out, cnt) if return_counts else out
