"""PointNetTrainer -- the training side of the reference's plain ``PointNet`` object (train_pointnet.py:31-111) on the GPU, and the
host staging of its cells.

One step is ``sess.run([net.class_acc, net.class_loss, net.train_op], feed)`` (:408).  It is sequenced here over the C-ABI entry
points, as the reference sequences it from Python; torch owns the buffers and computes nothing:

  forward    the convolutions a layer at a time with every layer kept (``lrg_pointwise_layer``), the cell's pooled row
             (``lrg_segmax``), t = conv_last - pooled (``lrg_pointnet_head_input``), the first fc layer as TWO products joined by
             ``lrg_gemm_f32``'s addend (conv[1] W0[c_last:] + bias, then + t W0[:c_last]: the concat of :61 is never written), each
             hidden fc layer's batch norm in training mode (``lrg_pointnet_bn_forward``: moments over the batch axis only, :92), the
             logits, the loss (``lrg_pointnet_softmax_ce_grad``).
  backward   dX = dZ W^T on ``lrg_gemm_f32``; dW = X^T dZ on ``lrg_gemm_f32_planes``: the reduction over the B * 1024 rows is cut
             into slices whose partial products are stored side by side and added in a fixed order (``lrg_segment_colsum``), not
             by atomic additions, so that a step gives the same bits every time; ``lrg_pointnet_bn_backward`` (the ReLU of :93 folded in);
             ``lrg_pointnet_head_input_backward`` (the single-winner gradient of tf.nn.max_pool2d, the last convolution's ReLU).
  update     ``lrg_pointnet_ema_update`` on the moving averages (:71-78), ``lrg_adam_step`` at the scheduled rate (:109-110).

``stage_cells`` and ``jitter`` are :327-350 and :235-246 on the host in NumPy with the script's own draws in the script's own order.
The flat parameter buffer, the Adam step, the staging of a batch, ``evaluate``, the checkpoint and the two ordered reductions over
the rows (``_dW``, ``_colsum`` over this trainer's own plan) are adam_trainer.py's.  DESIGN.md §3.13.  There is no CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _lib, checkpoint
from .adam_trainer import CellClassifierTrainer, variance_scaling_uniform
from .checkpoint import POINTNET_NUM_POINT as NUM_POINT, pointnet_bn_names, pointnet_variable_shapes, pointnet_variant
from .pointnet2 import _device, _ptr, _stream

ARCHITECTURES = {'today': ((64, 64, 64, 128, 1024), (512, 256)),          # NUM_FEATURE_CHANNELS, NUM_FC_CHANNELS of train_pointnet.py:20-22
                 'shipped': ((64, 64, 128, 512), (512,))}                  # models/pointnet_model5.ckpt.index


def learning_rate(step, base=2e-4, decay_steps=500, decay_rate=0.5):
    """tf.compat.v1.train.exponential_decay(base, step, decay_steps, decay_rate, staircase=True) (:109)."""
    return base * decay_rate ** (int(step) // int(decay_steps))


def trainable_names(conv_widths, fc_widths):
    """The trainables (:50-51, :66-69, :88-89, :96-97) in the order of the flat parameter buffer."""
    names = []
    for i in range(len(conv_widths)):
        names += ['kernel%d' % i, 'bias%d' % i]
    for j in range(len(fc_widths) + 1):
        names += ['fc_weights%d' % j, 'fc_bias%d' % j]
        if j < len(fc_widths):
            names += list(pointnet_bn_names(j)[:2])
    return names


def stage_cells(points, cls_id, area, rng):
    """The cells of one room as :327-350 stages them: (points [n, 2048, 6] in the file's dtype, labels [n, 2048]).  Cells of 1 m
    (3 m when the area's name contains 'kitti'), visited in the iteration order of the script's own set of tuples; x, y relative
    to the cell's centre and z to the cell's lowest point, subtracted in place on the file's dtype; 2048 rows drawn by
    ``rng.choice(n, 2048, replace=n < 2048)``.  rng: a numpy.random.RandomState (the script uses the module's global one)."""
    res = 3.0 if 'kitti' in str(area) else 1.0
    grid = np.round(points[:, :2] / res).astype(int)
    cells = set([tuple(g) for g in grid])                    # the same set, built the same way: its order is the script's
    out_p, out_l = [], []
    for g in cells:
        members = np.nonzero((grid[:, 0] == g[0]) & (grid[:, 1] == g[1]))[0]
        p = points[members, :6]
        low = p[:, 2].min()
        p[:, :2] -= np.array(g) * res
        p[:, 2] -= low
        subset = rng.choice(len(p), 2 * NUM_POINT, replace=len(p) < 2 * NUM_POINT)
        out_p.append(p[subset])
        out_l.append(cls_id[members][subset])
    return np.array(out_p), np.array(out_l)


def jitter(points, rng):
    """jitter_data (:235-246) on a batch [B, n, >= 3]: per cell, in this order, randint(2) mirrors x, randint(2) mirrors y,
    rand() * 0.5 + 0.75 scales and rand(3) * 0.4 - 0.2 shifts xyz.  Returns a copy in the input's dtype."""
    out = points.copy()
    for i in range(len(out)):
        if rng.randint(2):
            out[i, :, 0] = -out[i, :, 0]
        if rng.randint(2):
            out[i, :, 1] = -out[i, :, 1]
        scale = rng.rand() * 0.5 + 0.75
        shift = rng.rand(3) * 0.4 - 0.2
        out[i, :, :3] = out[i, :, :3] * scale + shift
    return out


def initial_weights(conv_widths, fc_widths, num_class, seed=0):
    """The state a fresh graph starts from (:50-51, :66-69, :71, :88-89, :96-97), name -> array in the TF shapes: kernels from
    VarianceScaling(1.0, fan_avg, uniform) -- U(-a, a), a = sqrt(6 / (fan_in + fan_out)), fans by TensorFlow's rule (the receptive
    field, every dimension but the last two, multiplies both: kernel0 [1,6,1,c] has fan_in 6 and fan_out 6 c) -- biases and beta 0,
    gamma 1, and both moving-average tables 0: ExponentialMovingAverage.apply on tensors starts its shadows at zero and does not
    debias, and the script is followed, not repaired.  The draws come from numpy.random.RandomState(seed): TensorFlow's own random
    stream cannot be reproduced, so the initial weights are the reference's in distribution only."""
    rs = np.random.RandomState(seed)
    w = {}
    for name, shp in pointnet_variable_shapes(conv_widths, fc_widths, num_class).items():
        if name.startswith('kernel') or name.startswith('fc_weights'):
            w[name] = variance_scaling_uniform(rs, shp)
        elif name.endswith('gamma'):
            w[name] = np.ones(shp, np.float32)
        else:
            w[name] = np.zeros(shp, np.float32)
    return w


class PointNetTrainer(CellClassifierTrainer):
    network = 'PointNet'
    checkpoint_tensors = staticmethod(checkpoint.pointnet_checkpoint_tensors)

    def __init__(self, batch_size, conv_widths=ARCHITECTURES['today'][0], fc_widths=ARCHITECTURES['today'][1], num_class=13, device=None,
                 base_learning_rate=2e-4, decay_steps=500, decay_rate=0.5, beta1=0.9, beta2=0.999, epsilon=1e-8, ema_decay=0.9):
        self.conv, self.fc, self.num_class = tuple(int(c) for c in conv_widths), tuple(int(c) for c in fc_widths), int(num_class)
        self.shapes = pointnet_variable_shapes(self.conv, self.fc, self.num_class)
        try:
            pointnet_variant(self.shapes)                    # the architectures the kernels run
        except checkpoint.BundleError as e:
            raise ValueError(str(e))
        if batch_size < 1:
            raise ValueError('batch_size must be at least 1')
        self.lib = _lib.load()
        self.dev = _device(device)
        self.B = int(batch_size)
        self.base_lr, self.decay_steps, self.decay_rate = base_learning_rate, decay_steps, decay_rate
        self.b1, self.b2, self.eps, self.ema_decay = beta1, beta2, epsilon, ema_decay
        self.names = trainable_names(self.conv, self.fc)
        self._plan = [(self.B, NUM_POINT), (1, self.B)]          # a column sum: per cell, then over the cells (one row at B = 1)

    # ---- variables ----
    def init_weights(self, seed=0):
        """Start from initial_weights(seed): the state a fresh graph starts from."""
        return self.load_weights(initial_weights(self.conv, self.fc, self.num_class, seed))

    def load_weights(self, weights):
        """weights: name -> array in the TF shapes under the names of checkpoint.pointnet_variable_shapes (the moving averages
        included).  Resets the optimiser (slots zero, step 0)."""
        self._check_weights(weights)
        dev, B, R = self.dev, self.B, self.B * NUM_POINT
        ema_names = [n for j in range(len(self.fc)) for n in pointnet_bn_names(j)[2:]]
        with torch.cuda.device(dev):
            self._bind(weights)
            # moving averages and the batch's moments: per block j mean [1024, c] then variance [1024, c], in both buffers
            self.ema = torch.from_numpy(np.concatenate([np.asarray(weights[k], np.float32).reshape(-1) for k in ema_names])).to(dev)
            self.moments = torch.zeros_like(self.ema)
            self.ema_views, self.moment_views = {}, {}
            o = 0
            for k in ema_names:
                n = int(np.prod(self.shapes[k]))
                self.ema_views[k] = self.ema[o:o + n].view(self.shapes[k])
                self.moment_views[k] = self.moments[o:o + n].view(self.shapes[k])
                o += n
            # activations, all kept for the backward pass
            f32 = dict(dtype=torch.float32, device=dev)
            self._x = torch.empty((R, 6), **f32)
            self._labels = torch.empty(R, dtype=torch.int32, device=dev)
            self._act = [torch.empty((R, c), **f32) for c in self.conv]
            self._pooled = torch.empty((B, self.conv[-1]), **f32)
            self._t = torch.empty((R, self.conv[-1]), **f32)
            self._z = [torch.empty((R, c), **f32) for c in self.fc]
            self._y = [torch.empty((R, c), **f32) for c in self.fc]
            self._logits = torch.empty((R, self.num_class), **f32)
            self._dlogits = torch.empty((R, self.num_class), **f32)
            wmax = max(self.conv + self.fc)
            self._dz = [torch.empty(R * wmax, **f32) for _ in range(2)]
            self._dskip = torch.empty((R, self.conv[1]), **f32)
            self._cs_part = [torch.empty(B * max(wmax, self.num_class), **f32)]
            dw = [(6 if i == 0 else self.conv[i - 1], c) for i, c in enumerate(self.conv)]
            dw += [(self.conv[-1], self.fc[0]), (self.conv[1], self.fc[0])]
            dw += [(k, n) for k, n in zip(self.fc, self.fc[1:] + (self.num_class,))]
            self._dw_part = torch.empty(max(self._dw_planes(k, n, R)[1] * k * n for k, n in dw), **f32)
            self._bn_ws_bytes = self.lib.lrg_pointnet_bn_backward_workspace_bytes(max(self.fc))
            self._bn_ws = torch.empty(self._bn_ws_bytes // 4, **f32)
            self._stats = torch.zeros(3, dtype=torch.float64, device=dev)
            torch.cuda.current_stream().synchronize()
        self._eval_net = None
        return self

    def weights_numpy(self):
        """name -> array in the TF shapes: the trainables and the moving averages (what PointNetHIP and write_bundle take)."""
        out = self._tf(self.views)
        out.update(self._tf(self.ema_views, list(self.ema_views)))
        return out

    def moments_numpy(self):
        """The last training batch's moments under the moving averages' names."""
        return self._tf(self.moment_views, list(self.moment_views))

    # ---- kernels ----
    def _gemm(self, M, N, K, A, lda, tA, B, ldb, tB, C, ldc, addend=None, mask=None):
        self._check(self.lib.lrg_gemm_f32(M, N, K, _ptr(A), lda, tA, _ptr(B), ldb, tB, _ptr(C), ldc, _ptr(addend), _ptr(mask), 1, _stream()),
                    'lrg_gemm_f32')

    def _layer(self, x, cin, w, ldw, bias, y, cout, relu):
        self._check(self.lib.lrg_pointwise_layer(_ptr(x), cin, _ptr(w), ldw, _ptr(bias), _ptr(y), self.B * NUM_POINT, cin, cout, relu, 0, 0, None,
                                                 0, _stream()), 'lrg_pointwise_layer')

    # ---- one step ----
    def backward(self, points, labels, loss_only=False, mark=None):
        """Forward in training mode (the batch's own moments), loss, accuracy, and -- unless loss_only -- the gradient of every
        trainable into the gradient buffer.  points [B,1024,6], labels [B,1024].  mark(name), if given, is called after each stage
        (tools/pointnet_train_bench.py records an event there)."""
        lib, B, R = self.lib, self.B, self.B * NUM_POINT
        conv, fc, nc, nf = self.conv, self.fc, len(self.conv), len(self.fc)
        c_last, c_skip = conv[-1], conv[1]
        V, G = self.views, self.gviews
        mark = mark or (lambda name: None)
        with torch.cuda.device(self.dev):
            st = _stream()
            self._upload(points, labels)
            # ---- :49-54 ----
            acts = [self._x] + self._act
            for i in range(nc):
                self._layer(acts[i], 6 if i == 0 else conv[i - 1], V['kernel%d' % i], conv[i], V['bias%d' % i], acts[i + 1], conv[i], 1)
            skip, last = acts[2], acts[nc]
            # ---- :56-61 ----
            self._check(lib.lrg_segmax(_ptr(last), _ptr(self._pooled), B, NUM_POINT, c_last, c_last, st), 'lrg_segmax')
            self._check(lib.lrg_pointnet_head_input(_ptr(last), _ptr(self._pooled), B, c_last, _ptr(self._t), st), 'lrg_pointnet_head_input')
            mark('conv')
            # ---- :86-99 ----
            W0 = V['fc_weights0']
            self._layer(skip, c_skip, W0[c_last:], fc[0], V['fc_bias0'], self._z[0], fc[0], 0)
            self._gemm(R, fc[0], c_last, self._t, c_last, 0, W0, fc[0], 0, self._z[0], fc[0], addend=self._z[0])
            for j in range(nf):
                beta, gamma, mean, var = pointnet_bn_names(j)
                if j > 0:
                    self._layer(self._y[j - 1], fc[j - 1], V['fc_weights%d' % j], fc[j], V['fc_bias%d' % j], self._z[j], fc[j], 0)
                self._check(lib.lrg_pointnet_bn_forward(_ptr(self._z[j]), _ptr(V[gamma]), _ptr(V[beta]), B, fc[j], _ptr(self._y[j]),
                                                        _ptr(self.moment_views[mean]), _ptr(self.moment_views[var]), st), 'lrg_pointnet_bn_forward')
            ncls = self.num_class
            self._layer(self._y[-1], fc[-1], V['fc_weights%d' % nf], ncls, V['fc_bias%d' % nf], self._logits, ncls, 0)
            mark('fc')
            # ---- :102-105 ----
            self._stats.zero_()
            self._check(lib.lrg_pointnet_softmax_ce_grad(_ptr(self._logits), _ptr(self._labels), R, ncls, None if loss_only else _ptr(self._dlogits),
                                                         _ptr(self._stats), st), 'lrg_pointnet_softmax_ce_grad')
            mark('loss')
            if loss_only:
                return self._scalars()
            # ---- the fc stack backwards ----
            cur, nxt = self._dz
            self._dW(self._y[-1], self._dlogits, fc[-1], ncls, R, G['fc_weights%d' % nf])
            self._colsum(self._dlogits, ncls, G['fc_bias%d' % nf], self._plan)
            self._gemm(R, fc[-1], ncls, self._dlogits, ncls, 0, V['fc_weights%d' % nf], ncls, 1, cur, fc[-1])
            for j in range(nf - 1, -1, -1):
                beta, gamma, mean, var = pointnet_bn_names(j)
                self._check(lib.lrg_pointnet_bn_backward(_ptr(self._z[j]), _ptr(self._y[j]), _ptr(cur), _ptr(self.moment_views[mean]),
                                                         _ptr(self.moment_views[var]), _ptr(V[gamma]), B, fc[j], _ptr(cur), _ptr(G[gamma]),
                                                         _ptr(G[beta]), _ptr(self._bn_ws), self._bn_ws_bytes, st), 'lrg_pointnet_bn_backward')
                self._colsum(cur, fc[j], G['fc_bias%d' % j], self._plan)
                if j > 0:
                    self._dW(self._y[j - 1], cur, fc[j - 1], fc[j], R, G['fc_weights%d' % j])
                    self._gemm(R, fc[j - 1], fc[j], cur, fc[j], 0, V['fc_weights%d' % j], fc[j], 1, nxt, fc[j - 1])
                    cur, nxt = nxt, cur
            # the first fc layer in its two blocks: rows [:c_last] read t, rows [c_last:] read conv[1]
            g0 = G['fc_weights0']
            self._dW(self._t, cur, c_last, fc[0], R, g0[:c_last])
            self._dW(skip, cur, c_skip, fc[0], R, g0[c_last:])
            self._gemm(R, c_skip, fc[0], cur, fc[0], 0, W0[c_last:], fc[0], 1, self._dskip, c_skip)
            self._gemm(R, c_last, fc[0], cur, fc[0], 0, W0, fc[0], 1, nxt, c_last)
            cur, nxt = nxt, cur
            mark('fc_backward')
            # ---- :56-59 backwards, with the last convolution's ReLU; the skip's gradient joins here when conv[1] is the last ----
            self._check(lib.lrg_pointnet_head_input_backward(_ptr(last), _ptr(self._pooled), _ptr(cur), _ptr(self._dskip) if nc == 2 else None, B,
                                                             c_last, 1, _ptr(cur), st), 'lrg_pointnet_head_input_backward')
            # ---- the convolutions backwards ----
            for i in range(nc - 1, -1, -1):
                K = 6 if i == 0 else conv[i - 1]
                self._dW(acts[i], cur, K, conv[i], R, G['kernel%d' % i])
                self._colsum(cur, conv[i], G['bias%d' % i], self._plan)
                if i > 0:
                    extra = self._dskip if (i == 2 and nc > 2) else None           # acts[2] = conv[1] also feeds the head
                    self._gemm(R, K, conv[i], cur, conv[i], 0, V['kernel%d' % i], conv[i], 1, nxt, K, addend=extra, mask=acts[i])
                    cur, nxt = nxt, cur
            mark('conv_backward')
            return self._scalars()

    def learning_rate(self):
        return learning_rate(self.step, self.base_lr, self.decay_steps, self.decay_rate)

    def train_step(self, points, labels, mark=None):
        """``sess.run([net.class_acc, net.class_loss, net.train_op], feed)`` (:408) -> dict(loss, acc)."""
        sc = self.backward(points, labels, mark=mark)
        with torch.cuda.device(self.dev):
            self._check(self.lib.lrg_pointnet_ema_update(_ptr(self.ema), _ptr(self.moments), self.ema.numel(),
                                                         ctypes.c_float(np.float32(1 - self.ema_decay)), _stream()), 'lrg_pointnet_ema_update')
            self._adam_update(self.learning_rate())
            if mark:
                mark('update')
        self._eval_net = None
        return sc

    def _inference_net(self):
        """PointNetHIP's two kernels on the current weights, the batch norm reading the moving averages."""
        from .pointnet import PointNetHIP
        return PointNetHIP(self.weights_numpy(), device=self.dev)
