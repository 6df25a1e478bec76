"""PointNet2Trainer -- the training side of the reference's ``PointNet2`` object (train_pointnet.py:113-211) on the GPU.

One step is ``sess.run([net.class_acc, net.class_loss, net.train_op], feed)`` (:408).  It is sequenced here over the C-ABI entry
points, as the reference sequences it from Python; torch owns the buffers and computes nothing:

  forward    PointNet2HIP's 25 launches with every layer kept: per set-abstraction level ``lrg_farthest_point_sample``,
             ``lrg_gather_point``, ``lrg_query_ball_point``, ``lrg_pointnet2_group_mlp_train`` (the grouped rows and the three layers'
             outputs); per feature-propagation level ``lrg_three_nn_interpolate`` (its indices and weights kept) and
             ``lrg_pointnet2_row_mlp_train``; the head; the loss (``lrg_pointnet_softmax_ce_grad``).  The logits carry the bits of the
             inference entry points.
  backward   only the features carry gradients (xyz is data; FPS, ball query and three_nn are index computations).  dX = dZ W^T on
             ``lrg_gemm_f32`` with the ReLU mask of the layer below; dW = X^T dZ on ``lrg_gemm_f32_planes`` + ``lrg_segment_colsum``
             and the bias gradients on ``lrg_segment_colsum`` alone: every reduction over the rows in slices added in a fixed order.
             The concat of a propagation level (:153) is two column blocks of the first layer's dX.  ``tf.reduce_max``'s gradient is
             ``lrg_pool_backward`` over segments of 32 rows.  The gradients of ``group_point`` and ``three_interpolate`` are
             ``lrg_pointnet2_scatter_grad``: every source row's sum in ascending entry order.  No float atomic anywhere, so a step
             gives the same bits every time.
  update     ``lrg_adam_step`` at the constant rate 0.001 (:210).

The gradient of l1_points .. l3_points has two contributors, added in this order: the skip connection of its propagation level
(written by the product), then the next level's grouping (the scatter's addend).  The flat parameter buffer, the Adam step, the staging of a batch, ``evaluate``, the checkpoint and the two ordered reductions over
the rows (``_dW``, ``_colsum`` over this trainer's own plan) are adam_trainer.py's.  DESIGN.md §3.14.  There is no CPU fallback.
"""
import ctypes
from math import gcd

import numpy as np
import torch

from . import _lib, checkpoint
from .adam_trainer import CellClassifierTrainer, variance_scaling_uniform
from .checkpoint import POINTNET2_FP_MLPS as FP_MLPS, POINTNET2_SA_MLPS as SA_MLPS, pointnet2_variable_shapes
from .pointnet2 import NSAMPLE, NUM_POINT, SA_LEVELS, _device, _ptr, _stream

LEARNING_RATE = 0.001            # train_pointnet.py:210
GEMM_ROWS = 65535 * 64           # lrg_gemm_f32: rows of one launch (64-row tiles on the grid's y axis)
POOL_GROUPS = 65535              # lrg_pool_backward: groups of one launch


def initial_weights(num_class=13, rgb_features=True, seed=0):
    """The state a fresh graph starts from (:133-134, :161-162, :194-200), name -> array in the TF shapes: kernels from
    VarianceScaling(1.0, fan_avg, uniform) with TensorFlow's fan rule (the receptive field multiplies both fans; it is 1 for every
    kernel of this network), biases 0 -- pointnet_train.initial_weights' rule.  The draws come from numpy.random.RandomState(seed):
    the initial weights are the reference's in distribution only."""
    rs = np.random.RandomState(seed)
    w = {}
    for name, shp in pointnet2_variable_shapes(num_class, rgb_features).items():
        if 'kernel' in name:
            w[name] = variance_scaling_uniform(rs, shp)
        else:
            w[name] = np.zeros(shp, np.float32)
    return w


def _widths(mlp):
    return np.array(mlp, dtype=np.int32)


def _colsum_plan(R):
    """[(segments, rows a segment)] of the stages that reduce R rows to one: segments of gcd(rows, 256) rows (doubled while a
    stage would have more than 65535 segments), until what is left has no such factor and is added in one stage."""
    plan = []
    while R > 1:
        s = gcd(R, 256)
        while R // s > 65535 and R % (2 * s) == 0:
            s *= 2
        if s == 1 or R // s > 65535:
            s = R
        plan.append((R // s, s))
        R //= s
    return plan or [(1, 1)]


class PointNet2Trainer(CellClassifierTrainer):
    network = 'PointNet2'
    checkpoint_tensors = staticmethod(checkpoint.pointnet2_checkpoint_tensors)

    def __init__(self, batch_size, num_class=13, rgb_features=True, device=None, learning_rate=LEARNING_RATE, beta1=0.9, beta2=0.999,
                 epsilon=1e-8):
        if batch_size < 1:
            raise ValueError('batch_size must be at least 1')
        if num_class < 1 or num_class > 512:
            raise ValueError('num_class must be in [1, 512]')
        self.lib = _lib.load()
        self.dev = _device(device)
        self.B, self.num_class, self.rgb_features = int(batch_size), int(num_class), bool(rgb_features)
        self.shapes = pointnet2_variable_shapes(self.num_class, self.rgb_features)
        self.names = list(self.shapes)
        self.lr, self.b1, self.b2, self.eps = learning_rate, beta1, beta2, epsilon
        self.npts = [NUM_POINT] + [m for m, _ in SA_LEVELS]                       # points of l0 .. l4
        self.feat = [3 if self.rgb_features else 0] + [m[-1] for m in SA_MLPS]    # feature widths of l0 .. l4

    # ---- variables ----
    def init_weights(self, seed=0):
        """Start from initial_weights(seed): the state a fresh graph starts from."""
        return self.load_weights(initial_weights(self.num_class, self.rgb_features, seed))

    def load_weights(self, weights):
        """weights: name -> array in the TF shapes of checkpoint.pointnet2_variable_shapes.  Resets the optimiser (slots zero, step 0)."""
        self._check_weights(weights)
        with torch.cuda.device(self.dev):
            self._bind(weights)
            if self.flat.data_ptr() % 16:
                raise _lib.LrgHipError('the parameter buffer is not 16-byte aligned')
            self._allocate()
            torch.cuda.current_stream().synchronize()
        self._eval_net = None
        self._packed_step = -1
        return self

    def _mlps(self):
        """(scope, layer ids, input width, widths) of the nine MLPs in forward order."""
        out = []
        for lv, mlp in enumerate(SA_MLPS):
            out.append(('layer%d/' % (lv + 1), range(3), 3 + self.feat[lv], mlp))
        up = self.feat[4]
        for lv, mlp in enumerate(FP_MLPS):
            out.append(('fa_layer%d/' % (lv + 1), range(len(mlp)), up + self.feat[3 - lv], mlp))
            up = mlp[-1]
        out.append(('', (1, 2), 128, (128, self.num_class)))
        return out

    def _allocate(self):
        dev, B, lib = self.dev, self.B, self.lib
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        self._x = torch.empty((B, NUM_POINT, 6), **f32)
        self._labels = torch.empty(B * NUM_POINT, **i32)
        self._xyz = [torch.empty((B, n, 3), **f32) for n in self.npts]
        self._feat = [torch.empty((B, NUM_POINT, 3), **f32) if self.rgb_features else None]
        self._feat += [torch.empty((B, self.npts[lv + 1], self.feat[lv + 1]), **f32) for lv in range(4)]
        self._dfeat = [None] + [torch.empty_like(t) for t in self._feat[1:]]
        self._fps = [torch.empty((B, self.npts[lv + 1]), **i32) for lv in range(4)]
        self._ball = [torch.empty((B, self.npts[lv + 1], NSAMPLE), **i32) for lv in range(4)]
        self._cnt = [torch.empty((B, self.npts[lv + 1]), **i32) for lv in range(4)]
        self._packed, big = [], []
        for scope, ids, cin, mlp in self._mlps():
            ks = [cin] + list(mlp[:-1])
            sizes = [lib.lrg_pointnet2_packed_floats(k, n) for k, n in zip(ks, mlp)]
            self._packed.append((torch.empty(sum(sizes), **f32), sizes, _widths(mlp), ks))
        # set abstraction: the grouped rows and the three layers of every level
        self._sa_rows, self._sa_keep = [], []
        for lv, mlp in enumerate(SA_MLPS):
            R = B * self.npts[lv + 1] * NSAMPLE
            self._sa_rows.append(torch.empty((R, 3 + self.feat[lv]), **f32))
            self._sa_keep.append([torch.empty((R, c), **f32) for c in mlp])
            big.append(R * max(max(mlp), 3 + self.feat[lv]))
        # feature propagation: indices, weights, the interpolated rows, the hidden layers and the output
        self._nn, self._nnw, self._interp, self._fp_keep, self._fp_out = [], [], [], [], []
        up = self.feat[4]
        for lv, mlp in enumerate(FP_MLPS):
            n = self.npts[3 - lv]
            self._nn.append(torch.empty((B, n, 3), **i32))
            self._nnw.append(torch.empty((B, n, 3), **f32))
            self._interp.append(torch.empty((B, n, up), **f32))
            self._fp_keep.append([torch.empty((B * n, c), **f32) for c in mlp[:-1]])
            self._fp_out.append(torch.empty((B, n, mlp[-1]), **f32))
            big.append(B * n * max(max(mlp), up))
            up = mlp[-1]
        R0 = B * NUM_POINT
        self._fc1 = torch.empty((R0, 128), **f32)
        self._logits = torch.empty((R0, self.num_class), **f32)
        self._dlogits = torch.empty((R0, self.num_class), **f32)
        big.append(R0 * max(128, self.num_class))
        self._dz = [torch.empty(max(big), **f32) for _ in range(2)]
        # weight gradients' planes and the column sums' partial rows
        dw, cs = [], []
        for (scope, ids, cin, mlp), R in zip(self._mlps(), self._mlp_rows()):
            for k, n in zip([cin] + list(mlp[:-1]), mlp):
                dw.append(self._dw_planes(k, n, R)[1] * k * n)
                cs.append(_colsum_plan(R)[0][0] * n)
        self._dw_part = torch.empty(max(dw), **f32)
        self._cs_part = [torch.empty(max(cs), **f32) for _ in range(2)]
        self._stats = torch.zeros(3, dtype=torch.float64, device=dev)

    def _mlp_rows(self):
        B = self.B
        return [B * self.npts[lv + 1] * NSAMPLE for lv in range(4)] + [B * self.npts[3 - lv] for lv in range(4)] + [B * NUM_POINT]

    def level_indices(self):
        """The index computations of the last forward as NumPy: dict(sa=[4 x dict(fps [B,m], idx [B,m,32])],
        fp=[4 x dict(nn_idx [B,n,3], weight [B,n,3])]), levels in forward order (fa_layer1 first)."""
        return dict(sa=[dict(fps=self._fps[lv].cpu().numpy(), idx=self._ball[lv].cpu().numpy()) for lv in range(4)],
                    fp=[dict(nn_idx=self._nn[lv].cpu().numpy(), weight=self._nnw[lv].cpu().numpy()) for lv in range(4)])

    # ---- kernels ----
    def _gemm(self, M, N, K, A, lda, B, ldb, C, ldc, mask=None):
        """C[M,N] = A[M,K] B[N,K]^T (dX = dZ W^T), zero where mask <= 0; launches of at most GEMM_ROWS rows."""
        at = lambda t, floats: ctypes.c_void_p(t.data_ptr() + 4 * floats)
        for r0 in range(0, M, GEMM_ROWS):
            rows = min(GEMM_ROWS, M - r0)
            self._check(self.lib.lrg_gemm_f32(rows, N, K, at(A, r0 * lda), lda, 0, _ptr(B), ldb, 1, at(C, r0 * ldc), ldc, None,
                                              at(mask, r0 * ldc) if mask is not None else None, 1, _stream()), 'lrg_gemm_f32')

    def _scatter(self, n, q, per, c, grad, ldg, col0, idx, weight, drop, addend, mask, out):
        self._check(self.lib.lrg_pointnet2_scatter_grad(self.B, n, q, per, c, _ptr(grad), ldg, col0, _ptr(idx), _ptr(weight), drop, _ptr(addend),
                                                        _ptr(mask), _ptr(out), _stream()), 'lrg_pointnet2_scatter_grad')

    def _pack(self):
        """The MFMA operand images of the current weights (once per update)."""
        if self._packed_step == self.step:
            return
        for (scope, ids, cin, mlp), (packed, sizes, _, ks) in zip(self._mlps(), self._packed):
            off = 0
            for i, k, n, size in zip(ids, ks, mlp, sizes):
                self._check(self.lib.lrg_pointnet2_pack_layer(k, n, _ptr(self.views['%skernel%d' % (scope, i)]), _ptr(self.views['%sbias%d' % (scope, i)]),
                                                              _ptr(packed[off:]), _stream()), 'lrg_pointnet2_pack_layer')
                off += size
        self._packed_step = self.step

    def _forward(self, mark):
        lib, B, st = self.lib, self.B, _stream()
        wp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        self._pack()
        self._xyz[0].copy_(self._x[:, :, :3])
        if self.rgb_features:
            self._feat[0].copy_(self._x[:, :, 3:])
        mark('upload')
        for lv, (m, radius) in enumerate(SA_LEVELS):
            n, c = self.npts[lv], self.feat[lv]
            xyz, new_xyz = self._xyz[lv], self._xyz[lv + 1]
            self._check(lib.lrg_farthest_point_sample(B, n, m, _ptr(xyz), None, _ptr(self._fps[lv]), st), 'lrg_farthest_point_sample')
            mark('fps')
            self._check(lib.lrg_gather_point(B, n, m, _ptr(xyz), _ptr(self._fps[lv]), _ptr(new_xyz), st), 'lrg_gather_point')
            self._check(lib.lrg_query_ball_point(B, n, m, ctypes.c_float(radius), NSAMPLE, _ptr(xyz), _ptr(new_xyz), _ptr(self._ball[lv]),
                                                 _ptr(self._cnt[lv]), st), 'lrg_query_ball_point')
            mark('ball_query')
            packed, _, widths, _ = self._packed[lv]
            keep = self._sa_keep[lv]
            self._check(lib.lrg_pointnet2_group_mlp_train(B, n, m, NSAMPLE, c, _ptr(xyz), _ptr(new_xyz), _ptr(self._feat[lv]), _ptr(self._ball[lv]),
                                                          wp(widths), _ptr(packed), _ptr(self._feat[lv + 1]), _ptr(self._sa_rows[lv]), _ptr(keep[0]),
                                                          _ptr(keep[1]), _ptr(keep[2]), st), 'lrg_pointnet2_group_mlp_train')
            mark('sa_forward')
        up = self._feat[4]
        for lv, mlp in enumerate(FP_MLPS):
            dst = 3 - lv
            n, m, c = self.npts[dst], self.npts[dst + 1], up.shape[2]
            self._check(lib.lrg_three_nn_interpolate(B, n, m, c, _ptr(self._xyz[dst]), _ptr(self._xyz[dst + 1]), _ptr(up), None, _ptr(self._nn[lv]),
                                                     _ptr(self._nnw[lv]), _ptr(self._interp[lv]), st), 'lrg_three_nn_interpolate')
            packed, _, widths, _ = self._packed[4 + lv]
            skip = self._feat[dst]
            keep = self._fp_keep[lv] + [None] * 3
            self._check(lib.lrg_pointnet2_row_mlp_train(B * n, c, 0 if skip is None else skip.shape[2], _ptr(self._interp[lv]), _ptr(skip), len(mlp),
                                                        wp(widths), 1, _ptr(packed), _ptr(self._fp_out[lv]), _ptr(keep[0]), _ptr(keep[1]), _ptr(keep[2]),
                                                        st), 'lrg_pointnet2_row_mlp_train')
            up = self._fp_out[lv]
            mark('fp_forward')
        packed, _, widths, _ = self._packed[8]
        self._check(lib.lrg_pointnet2_row_mlp_train(B * NUM_POINT, 128, 0, _ptr(up), None, 2, wp(widths), 0, _ptr(packed), _ptr(self._logits),
                                                    _ptr(self._fc1), None, None, st), 'lrg_pointnet2_row_mlp_train')
        mark('fp_forward')

    # ---- one step ----
    def backward(self, points, labels, loss_only=False, mark=None):
        """Forward with every layer kept, loss, accuracy, and -- unless loss_only -- the gradient of every trainable into the gradient
        buffer.  points [B,1024,6], labels [B,1024].  mark(name), if given, is called after each stage
        (tools/pointnet2_train_bench.py records an event there)."""
        lib, B = self.lib, self.B
        V, G = self.views, self.gviews
        mark = mark or (lambda name: None)
        ncls, R0 = self.num_class, self.B * NUM_POINT
        with torch.cuda.device(self.dev):
            st = _stream()
            self._upload(points, labels)
            self._forward(mark)
            self._stats.zero_()
            self._check(lib.lrg_pointnet_softmax_ce_grad(_ptr(self._logits), _ptr(self._labels), R0, ncls, None if loss_only else _ptr(self._dlogits),
                                                         _ptr(self._stats), st), 'lrg_pointnet_softmax_ce_grad')
            mark('loss')
            if loss_only:
                return self._scalars()
            cur, nxt = self._dz
            # ---- the head (:193-202) ----
            fp4 = self._fp_out[3].view(R0, 128)
            self._dW(self._fc1, self._dlogits, 128, ncls, R0, G['kernel2'])
            self._colsum(self._dlogits, ncls, G['bias2'], _colsum_plan(R0))
            self._gemm(R0, 128, ncls, self._dlogits, ncls, V['kernel2'], ncls, cur, 128, mask=self._fc1)
            self._dW(fp4, cur, 128, 128, R0, G['kernel1'])
            self._colsum(cur, 128, G['bias1'], _colsum_plan(R0))
            self._gemm(R0, 128, 128, cur, 128, V['kernel1'], 128, nxt, 128, mask=fp4)
            cur, nxt = nxt, cur
            mark('head_backward')
            # ---- feature propagation, fa_layer4 first: cur is the gradient of the level's last pre-activation ----
            for lv in range(3, -1, -1):
                dst, mlp, scope = 3 - lv, FP_MLPS[lv], 'fa_layer%d/' % (lv + 1)
                n, m = self.npts[dst], self.npts[dst + 1]
                R = B * n
                for i in range(len(mlp) - 1, 0, -1):
                    X, k = self._fp_keep[lv][i - 1], mlp[i - 1]
                    self._dW(X, cur, k, mlp[i], R, G['%skernel%d' % (scope, i)])
                    self._colsum(cur, mlp[i], G['%sbias%d' % (scope, i)], _colsum_plan(R))
                    self._gemm(R, k, mlp[i], cur, mlp[i], V['%skernel%d' % (scope, i)], mlp[i], nxt, k, mask=X)
                    cur, nxt = nxt, cur
                c_up, c_skip, w0 = self._interp[lv].shape[2], self.feat[dst], mlp[0]
                W0, G0 = V[scope + 'kernel0'], G[scope + 'kernel0']
                self._dW(self._interp[lv], cur, c_up, w0, R, G0[:c_up])
                if c_skip:
                    self._dW(self._feat[dst], cur, c_skip, w0, R, G0[c_up:])
                self._colsum(cur, w0, G[scope + 'bias0'], _colsum_plan(R))
                if dst >= 1:                                                   # the skip's block: the first contributor of l<dst>_points
                    self._gemm(R, c_skip, w0, cur, w0, W0[c_up:], w0, self._dfeat[dst].view(-1), c_skip)
                self._gemm(R, c_up, w0, cur, w0, W0, w0, nxt, c_up)            # the interpolated block
                mark('fp_backward')
                below = self._fp_out[lv - 1] if lv > 0 else None               # what was interpolated: an FP output (ReLU) or l4_points
                self._scatter(m, n, 3, c_up, nxt, c_up, 0, self._nn[lv], self._nnw[lv], 1, None, below,
                              cur if lv > 0 else self._dfeat[4])
                mark('scatter')
            # ---- set abstraction, layer4 first ----
            for lv in range(3, -1, -1):
                scope, (w1, w2, w3) = 'layer%d/' % (lv + 1), SA_MLPS[lv]
                n, m, c = self.npts[lv], self.npts[lv + 1], self.feat[lv]
                groups, k0 = B * m, 3 + c
                R = groups * NSAMPLE
                keep, dpool = self._sa_keep[lv], self._dfeat[lv + 1].view(groups, w3)
                for g0 in range(0, groups, POOL_GROUPS):
                    gs = min(POOL_GROUPS, groups - g0)
                    self._check(lib.lrg_pool_backward(_ptr(keep[2][g0 * NSAMPLE:]), _ptr(dpool[g0:]), gs, NSAMPLE, w3, w3,
                                                      _ptr(cur[g0 * NSAMPLE * w3:]), st), 'lrg_pool_backward')
                for i, (X, k, wd) in ((2, (keep[1], w2, w3)), (1, (keep[0], w1, w2))):
                    self._dW(X, cur, k, wd, R, G['%skernel%d' % (scope, i)])
                    self._colsum(cur, wd, G['%sbias%d' % (scope, i)], _colsum_plan(R))
                    self._gemm(R, k, wd, cur, wd, V['%skernel%d' % (scope, i)], wd, nxt, k, mask=X)
                    cur, nxt = nxt, cur
                self._dW(self._sa_rows[lv], cur, k0, w1, R, G[scope + 'kernel0'])
                self._colsum(cur, w1, G[scope + 'bias0'], _colsum_plan(R))
                mark('sa_backward')
                if lv >= 1:                                                    # layer1's inputs are data
                    self._gemm(R, k0, w1, cur, w1, V[scope + 'kernel0'], w1, nxt, k0)
                    mark('sa_backward')
                    self._scatter(n, m * NSAMPLE, 1, c, nxt, k0, 3, self._ball[lv], None, 0, self._dfeat[lv], None, self._dfeat[lv])
                    mark('scatter')
            return self._scalars()

    def train_step(self, points, labels, mark=None):
        """``sess.run([net.class_acc, net.class_loss, net.train_op], feed)`` (:408) -> dict(loss, acc)."""
        sc = self.backward(points, labels, mark=mark)
        with torch.cuda.device(self.dev):
            self._adam_update(self.lr)
            if mark:
                mark('update')
        self._eval_net = None
        return sc

    def train_logits(self):
        """The logits [B,1024,num_class] (a device tensor) of the last backward / train_step's forward."""
        return self._logits.view(self.B, NUM_POINT, self.num_class)

    def _inference_net(self):
        from .pointnet2 import PointNet2HIP
        return PointNet2HIP(self.weights_numpy(), device=self.dev)
