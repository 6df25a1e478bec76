"""What the trainers share (train.py, pointnet_train.py, pointnet2_train.py, mcpnet_train.py), on two levels and nothing else.

``AdamTrainer``              every trainable in one flat float32 buffer with its gradient and Adam's two slots beside it, the NumPy
                             views out of them, the step counter and the one call of ``lrg_adam_step``.
``CellClassifierTrainer``    on top of it, what the two classifiers of 1024-point cells have in common: staging a batch, loss and
                             accuracy out of ``lrg_pointnet_softmax_ce_grad``'s sums, the validation pass through the inference
                             network, the checkpoint, and the two reductions over the rows that neither adds atomically: dW = X^T dZ in
                             planes, a column sum in the stages of a plan.

Nothing here chooses a summation order: the slices of a weight gradient follow from the shapes, and the stages of a column sum are
the caller's plan, which differs between the two trainers and is part of their arithmetic.  torch owns the buffers; it computes nothing.
"""
import ctypes

import numpy as np
import torch

from . import _lib, checkpoint
from .pointnet2 import NUM_POINT, _ptr, _stream

DW_WORKGROUPS = 2048             # a weight gradient's reduction over the rows is cut until about this many workgroups share it


def variance_scaling_uniform(rs, shape):
    """A kernel of TF shape `shape` from VarianceScaling(1.0, fan_avg, uniform): U(-a, a), a = sqrt(6 / (fan_in + fan_out)), fans by
    TensorFlow's rule (the receptive field, every dimension but the last two, multiplies both), drawn from the RandomState rs."""
    field = int(np.prod(shape[:-2]))
    lim = np.sqrt(6.0 / (field * shape[-2] + field * shape[-1]))
    return rs.uniform(-lim, lim, shape).astype(np.float32)


class AdamTrainer:
    """A subclass sets lib, dev, b1, b2, eps, shapes (name -> TF shape) and names (the trainables in the buffer's order), then calls
    _bind; it launches on dev's current stream with dev current."""
    step = 0
    flat = None

    def _bind(self, weights):
        """weights: name -> array of the variable's size.  Fills flat, zeroes the gradient and the slots, cuts views / gviews (kernels
        as [cin, cout]) and resets the step."""
        sizes = [int(np.prod(self.shapes[k])) for k in self.names]
        self.offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        host = np.concatenate([np.asarray(weights[k], np.float32).reshape(-1) for k in self.names])
        self.flat = torch.from_numpy(host).to(self.dev)
        self.gflat = torch.zeros_like(self.flat)
        self.m = torch.zeros_like(self.flat)
        self.v = torch.zeros_like(self.flat)
        self.views, self.gviews = {}, {}
        for k, o, n in zip(self.names, self.offs[:-1], sizes):
            shp = self.shapes[k]
            shp2 = (shp[-1],) if len(shp) == 1 else (int(np.prod(shp[:-1])), shp[-1])
            self.views[k] = self.flat[o:o + n].view(shp2)
            self.gviews[k] = self.gflat[o:o + n].view(shp2)
        self.step = 0

    def _tf(self, views, names=None):
        return {k: views[k].cpu().numpy().reshape(self.shapes[k]) for k in (self.names if names is None else names)}

    def weights_numpy(self):
        """name -> array in the TF shapes."""
        return self._tf(self.views)

    def grads_numpy(self):
        return self._tf(self.gviews)

    def slots_numpy(self):
        """(m, v): Adam's slots of the trainables in the TF shapes."""
        def cut(buf):
            return {k: buf[o:o + self.views[k].numel()].cpu().numpy().reshape(self.shapes[k]) for k, o in zip(self.names, self.offs[:-1])}
        return cut(self.m), cut(self.v)

    def _adam_update(self, lr):
        """Step `step + 1` of Adam at the rate lr, bias-corrected as AdamOptimizer corrects it, on the whole buffer."""
        self.step += 1
        lr_t = lr * np.sqrt(1.0 - self.b2 ** self.step) / (1.0 - self.b1 ** self.step)
        _lib.check(self.lib.lrg_adam_step(_ptr(self.flat), _ptr(self.gflat), _ptr(self.m), _ptr(self.v), self.flat.numel(), ctypes.c_float(lr_t),
                                          ctypes.c_float(self.b1), ctypes.c_float(self.b2), ctypes.c_float(self.eps), _stream()), 'lrg_adam_step')


class CellClassifierTrainer(AdamTrainer):
    """A subclass also sets B, num_class, network (its name in messages), checkpoint_tensors (the checkpoint.py function of its Saver
    layout), the buffers _x, _labels, _stats, _dw_part and _cs_part, and _inference_net()."""
    _eval_net = None

    def _check(self, rc, what):
        _lib.check(rc, what)

    def _check_weights(self, weights):
        for k, shp in self.shapes.items():
            if k not in weights:
                raise KeyError('%s weight %s missing' % (self.network, k))
            if tuple(np.shape(weights[k])) != tuple(shp):
                raise ValueError('%s has shape %s, %s needs %s' % (k, np.shape(weights[k]), self.network, shp))

    def checkpoint_numpy(self):
        """Everything the reference's ``Saver`` (:367, :438) stores: the network's ``*_checkpoint_tensors`` of checkpoint.py."""
        m, v = self.slots_numpy()
        return self.checkpoint_tensors(self.weights_numpy(), m, v, self.step, self.b1, self.b2)

    def save(self, prefix):
        checkpoint.write_bundle(prefix, self.checkpoint_numpy())

    # ---- the reductions over the rows ----
    def _dw_planes(self, K, N, R):
        """Into how many slices the R rows of a [K, N] weight gradient are cut: enough for about DW_WORKGROUPS workgroups of 64 x 64
        tiles, never under 256 rows a slice.  A function of the shapes alone, so a step always adds in the same order."""
        tiles = -(-K // 64) * -(-N // 64)
        split = max(1, min(R // 256, -(-DW_WORKGROUPS // tiles)))
        return split, self.lib.lrg_gemm_f32_planes_count(R, split)

    def _dW(self, X, dZ, K, N, R, out):
        """out[K,N] = X[R,K]^T dZ[R,N]: the rows cut into slices whose partial products are stored side by side
        (lrg_gemm_f32_planes) and then added in ascending order (lrg_segment_colsum); nothing is added atomically."""
        split, planes = self._dw_planes(K, N, R)
        self._check(self.lib.lrg_gemm_f32_planes(K, N, R, _ptr(X), K, 1, _ptr(dZ), N, 0, _ptr(self._dw_part), split, _stream()),
                    'lrg_gemm_f32_planes')
        self._check(self.lib.lrg_segment_colsum(_ptr(self._dw_part), 1, planes, K * N, _ptr(out), _stream()), 'lrg_segment_colsum')

    def _colsum(self, x, N, out, plan):
        """out[N] = the column sums of x[R,N] in the stages [(segments, rows a segment)] of the caller's plan, each in ascending row
        order; a stage's partial rows go to _cs_part[0] and [1] in turn (a plan of two stages needs only the first)."""
        src = x
        for i, (segs, rows) in enumerate(plan):
            dst = out if i == len(plan) - 1 else self._cs_part[i & 1]
            self._check(self.lib.lrg_segment_colsum(_ptr(src), segs, rows, N, _ptr(dst), _stream()), 'lrg_segment_colsum')
            src = dst

    # ---- a batch in, its scalars out ----
    def _upload(self, points, labels):
        points = np.ascontiguousarray(points, dtype=np.float32)
        if points.shape != (self.B, NUM_POINT, 6):
            raise ValueError('points must be [%d, %d, 6]' % (self.B, NUM_POINT))
        labels = np.asarray(labels)
        if labels.shape != (self.B, NUM_POINT):
            raise ValueError('labels must be [%d, %d]' % (self.B, NUM_POINT))
        self._x.copy_(torch.from_numpy(points).view(self._x.shape))
        self._labels.copy_(torch.from_numpy(np.ascontiguousarray(labels.astype(np.int32))).view(-1))

    def _scalars(self, stats=None, rows=None):
        """dict(loss, acc) from lrg_pointnet_softmax_ce_grad's sums (default: the training batch's)."""
        s = (self._stats if stats is None else stats).cpu().numpy()
        if s[2]:
            raise ValueError('%d labels are outside [0, %d)' % (int(s[2]), self.num_class))
        rows = self.B * NUM_POINT if rows is None else rows
        return dict(loss=float(s[0] / rows), acc=float(s[1] / rows))

    def eval_logits(self, points):
        """The logits [b,1024,num_class] (a device tensor) of the validation loop (``is_training_pl: False``, :432): the inference
        network on the trainer's current weights, built once per update.  Any number of cells, all in one pass."""
        if self._eval_net is None:
            self._eval_net = self._inference_net()
        points = np.ascontiguousarray(points, dtype=np.float32)
        with torch.cuda.device(self.dev):
            return self._eval_net._forward(torch.from_numpy(points).to(self.dev))

    def evaluate(self, points, labels):
        """dict(loss, acc) of a batch in the validation loop (:419-436)."""
        labels = np.ascontiguousarray(np.asarray(labels).astype(np.int32)).reshape(-1)
        with torch.cuda.device(self.dev):
            out = self.eval_logits(points)
            rows = out.shape[0] * NUM_POINT
            if labels.size != rows:
                raise ValueError('labels must be [%d, %d]' % (out.shape[0], NUM_POINT))
            lab = torch.from_numpy(labels).to(self.dev)
            stats = torch.zeros(3, dtype=torch.float64, device=self.dev)
            self._check(self.lib.lrg_pointnet_softmax_ce_grad(_ptr(out), _ptr(lab), rows, self.num_class, None, _ptr(stats), _stream()),
                        'lrg_pointnet_softmax_ce_grad')
            return self._scalars(stats, rows)
