"""The plain PointNet, the learned baseline of the reference's ``benchmarks.py --mode pointnet`` (network: train_pointnet.py:31-99),
on the GPU.

Everything around the network is the PointNet2 mode's and is imported from ``pointnet2``, not copied: ``prepare_room``
(benchmarks.py:199-215), ``cells`` / ``cell_inputs`` (:283-295), ``grid_resolution`` (:283) and ``segment`` (:300-306, :405-416).

``fold_batch_norm``  the batch norm after a hidden fc layer at inference (``is_training_pl: False``, :296): its moments run over the
                     batch axis only (:92), so the moving averages are [1024, c] tables and the layer is a scale and a shift per
                     (row position, channel).
``PointNetHIP``      the network in two launches per pass (csrc/lrg_pointnet.hip): ``lrg_pointnet_features`` (the convolutions, the
                     skip rows and the cell's pooled row) and ``lrg_pointnet_head`` (the fc layers on
                     concat(conv_last - pooled, conv[1])).  The architecture is read from the weights' shapes
                     (checkpoint.pointnet_variant): the shipped pointnet_model5 and the network train_pointnet.py builds today
                     differ, and both run.

There is no CPU fallback: without the library or a GPU, ``_lib.LrgHipError`` is raised.  DESIGN.md §3.12.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .checkpoint import BundleError, pointnet_bn_names, pointnet_variable_shapes, pointnet_variant
from .pointnet2 import (NUM_POINT, _device, _ptr, _stream, cell_inputs, cells, classify_cells, classify_rooms, grid_resolution,  # noqa: F401
                        prepare_room, segment)

BN_EPSILON = 1e-3            # train_pointnet.py:83
CHUNK_CELLS = 64             # cells per pass through the network (PointNetHIP.logits)


def fold_batch_norm(beta, gamma, mean, variance):
    """-> (scale, shift) float32 [1024, c] with normed = x * scale + shift: tf.nn.batch_normalization's own order,
    scale = rsqrt(variance + 1e-3) * gamma, shift = beta - mean * scale, every step rounded to float32."""
    f = np.float32
    mean, variance = np.asarray(mean, f), np.asarray(variance, f)
    scale = (f(1) / np.sqrt(variance + f(BN_EPSILON))) * np.asarray(gamma, f)[None, :]
    shift = np.asarray(beta, f)[None, :] - mean * scale
    return np.ascontiguousarray(scale, f), np.ascontiguousarray(shift, f)


class PointNetHIP:
    """PointNet (train_pointnet.py:31-99) at inference on gfx950.  weights: name -> array in the TF shapes under the names of
    checkpoint.pointnet_variable_shapes (checkpoint.load_pointnet_weights).  conv_widths, fc_widths (the hidden fc layers) and
    num_class are read from the shapes."""

    def __init__(self, weights, device=None):
        self.lib = _lib.load()
        self.device = _device(device)
        try:
            self.conv_widths, self.fc_widths, self.num_class = pointnet_variant({k: np.shape(v) for k, v in weights.items()})
        except BundleError as e:
            raise ValueError(str(e))
        for k, shp in pointnet_variable_shapes(self.conv_widths, self.fc_widths, self.num_class).items():
            if k not in weights:
                raise KeyError('PointNet weight %s missing' % k)
            if tuple(np.shape(weights[k])) != tuple(shp):
                raise ValueError('%s has shape %s, PointNet needs %s' % (k, np.shape(weights[k]), shp))
        self._conv = np.array(self.conv_widths, dtype=np.int32)
        self._fc = np.array(self.fc_widths + (self.num_class,), dtype=np.int32)
        tables = []
        for j in range(len(self.fc_widths)):
            tables.extend(fold_batch_norm(*(weights[n] for n in pointnet_bn_names(j))))
        with torch.cuda.device(self.device):
            self.conv_packed = self._pack(weights, 'kernel%d', 'bias%d', len(self.conv_widths))
            self.fc_packed = self._pack(weights, 'fc_weights%d', 'fc_bias%d', len(self._fc))
            self.bn = torch.from_numpy(np.concatenate([t.reshape(-1) for t in tables])).to(self.device)
            torch.cuda.current_stream().synchronize()

    def _pack(self, weights, kernel, bias, count):
        layers = []
        for i in range(count):
            w = np.ascontiguousarray(weights[kernel % i], dtype=np.float32)
            layers.append((w.reshape(-1, w.shape[-1]), np.ascontiguousarray(weights[bias % i], dtype=np.float32)))     # kernel0 [1,6,1,c] -> [6, c]
        sizes = [self.lib.lrg_pointnet_packed_floats(w.shape[0], w.shape[1]) for w, _ in layers]
        packed = torch.empty(sum(sizes), dtype=torch.float32, device=self.device)
        off = 0
        for (w, b), size in zip(layers, sizes):
            wd, bd = torch.from_numpy(w).to(self.device), torch.from_numpy(b).to(self.device)
            _lib.check(self.lib.lrg_pointnet_pack_layer(w.shape[0], w.shape[1], _ptr(wd), _ptr(bd), _ptr(packed[off:]), _stream()),
                       'lrg_pointnet_pack_layer')
            off += size
        torch.cuda.current_stream().synchronize()                    # wd, bd may go
        return packed

    def _forward(self, x, parts=None, mark=None):
        """x [b, 1024, 6] float32 on the device -> logits [b, 1024, num_class]: two launches (and the memset of the pooled rows),
        whatever b is.  parts, if a dict, receives the device tensors skip, last and pooled; mark(name), if given, is called after
        each launch (tools/pointnet_bench.py records an event there)."""
        b = x.shape[0]
        c_skip, c_last = self.conv_widths[1], self.conv_widths[-1]
        skip = torch.empty((b, NUM_POINT, c_skip), dtype=torch.float32, device=x.device)
        last = torch.empty((b, NUM_POINT, c_last), dtype=torch.float32, device=x.device)
        pooled = torch.empty((b, c_last), dtype=torch.float32, device=x.device)
        out = torch.empty((b, NUM_POINT, self.num_class), dtype=torch.float32, device=x.device)
        i32p = ctypes.POINTER(ctypes.c_int32)
        _lib.check(self.lib.lrg_pointnet_features(b, len(self._conv), self._conv.ctypes.data_as(i32p), _ptr(x), _ptr(self.conv_packed), _ptr(skip),
                                                  _ptr(last), _ptr(pooled), _stream()), 'lrg_pointnet_features')
        if mark:
            mark('features')
        _lib.check(self.lib.lrg_pointnet_head(b, c_last, c_skip, _ptr(last), _ptr(skip), _ptr(pooled), len(self._fc), self._fc.ctypes.data_as(i32p),
                                              _ptr(self.fc_packed), _ptr(self.bn), _ptr(out), _stream()), 'lrg_pointnet_head')
        if mark:
            mark('head')
        if parts is not None:
            parts.update(skip=skip, last=last, pooled=pooled)
        return out

    def logits(self, batch, return_parts=False):
        """batch [B, 1024, 6] float32 (cell_inputs) -> float32 [B, 1024, num_class].  With return_parts also dict(skip
        [B,1024,conv[1]], last [B,1024,conv[-1]], pooled [B,conv[-1]]) of NumPy arrays.

        More than CHUNK_CELLS = 64 cells are processed 64 at a time.  Per cell the pass holds the input 6 K floats (K = 1024),
        the skip rows 64 K, the last convolution's rows up to 1024 K and the logits num_class K (260 K for kitti): 5.4 MB at
        most, 350 MB a pass.  Both kernels work on one cell at a time, so the result does not depend on the chunking."""
        batch = np.ascontiguousarray(batch, dtype=np.float32)
        if batch.ndim != 3 or batch.shape[1:] != (NUM_POINT, 6):
            raise ValueError('batch must be [B, %d, 6]' % NUM_POINT)
        out = np.empty((len(batch), NUM_POINT, self.num_class), dtype=np.float32)
        chunks = []
        with torch.cuda.device(self.device):
            for c0 in range(0, len(batch), CHUNK_CELLS):
                parts = {} if return_parts else None
                out[c0:c0 + CHUNK_CELLS] = self._forward(torch.from_numpy(batch[c0:c0 + CHUNK_CELLS]).to(self.device), parts).cpu().numpy()
                if return_parts:
                    chunks.append({k: v.cpu().numpy() for k, v in parts.items()})
        if not return_parts:
            return out
        c_skip, c_last = self.conv_widths[1], self.conv_widths[-1]
        empty = dict(skip=np.zeros((0, NUM_POINT, c_skip), np.float32), last=np.zeros((0, NUM_POINT, c_last), np.float32),
                     pooled=np.zeros((0, c_last), np.float32))
        return out, {k: np.concatenate([ch[k] for ch in chunks]) if chunks else empty[k] for k in empty}

    def classify_cells(self, batch):
        """batch [B, 1024, 6] -> int32 [B, 1024]: the argmax of every row's logits on the device, a tie to the lowest class as
        numpy.argmax (benchmarks.py:297)."""
        return classify_cells(self, batch, CHUNK_CELLS)

    def classify(self, rooms, area=None, grid_resolution_m=None):
        """class_labels of every room (benchmarks.py:282-298), PointNet2HIP.classify's contract: rooms are dicts with 'points'
        (equalised: prepare_room) or [N, >= 6] arrays; the cells of ALL rooms go through the network together.  area picks the cell
        size as :283 does (or give grid_resolution_m).  Returns one int32 array per room."""
        return classify_rooms(self, rooms, area, grid_resolution_m)
