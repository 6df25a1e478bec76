"""Training MCPNet on the GPU: the job of the reference's train_mcpnet.py (network learn_region_grow_util.py:191-232, loss
metric_loss_ops.py:157-236).  DESIGN.md §3.17.

The network trained is the one the shipped models/mcpnet_model5.ckpt holds and test_mcpnet.py evaluates: feature_size = 6, so
``neighbor_pl`` is the staged ``neighbor_points[..., :6]`` and ``input_pl`` the staged ``points`` (z, r, g, b).  train_mcpnet.py as
it stands (feature_size = 3, the rows fed to input_pl) does not run against that class.

``MCPNetTrainer``     one step = repack (``lrg_mcp_pack_weights``) -> the forward pass that keeps its layers (``lrg_mcp_embed_train``)
                      -> ``lrg_mcp_triplet_semihard`` (loss, dD, dfc4) -> the backward pass on lrg_train.hip's kernels (``lrg_gemm_f32``
                      with the ReLU mask for every dX, ``lrg_gemm_f32_planes`` + ``lrg_segment_colsum`` for every dW and bias,
                      ``lrg_pool_backward`` for the max over the 50 rows) -> ``lrg_adam_step`` at 0.001.  Nothing is added atomically:
                      a step gives the same bits every time.  torch owns the buffers; it computes nothing.
``stage_room`` / ``stage_area``   the stage_data block (:78-143) on ``mcpnet.prepare_room`` / ``mcpnet.neighbors(rng='legacy')``; the
                      512-point blocks are carved on the host in the script's order.
``even_sampling``, ``nn_accuracy``, ``anova``   get_even_sampling, get_acc, get_anova (:26-68).

A batch without a positive pair makes the reference divide 0 by 0 and push NaN through Adam; here ``train_step`` returns
loss = nan, applies no update and counts the batch in ``skipped_batches``.
There is no CPU fallback: without the library or a GPU, ``_lib.LrgHipError`` is raised.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib, checkpoint, h5lite, mcpnet
from .adam_trainer import DW_WORKGROUPS, AdamTrainer, variance_scaling_uniform
from .checkpoint import MCPNET_SHAPES
from .mcpnet import EMBEDDING_SIZE, NUM_NEIGHBORS, _device, _ptr, _stream

BATCH_SIZE = 256                 # train_mcpnet.py:17
SAMPLES_PER_INSTANCE = 16        # :23
LOCAL_RANGE = 2                  # :13
HIDDEN = 200                     # :18
MAX_EPOCH = 50                   # :22
BLOCK = 2 * BATCH_SIZE           # a staged block: batch_size * 2 points (:130)
NAMES = ('mcp_kernel1', 'mcp_bias1', 'mcp_kernel2', 'mcp_bias2', 'mcp_kernel3', 'mcp_bias3', 'mcp_kernel4', 'mcp_bias4')
MAX_BATCH = 1024                 # LRG_MCP_TRIPLET_MAX_B


def initial_weights(seed=0):
    """A fresh graph's state (learn_region_grow_util.py:198-205): kernels from VarianceScaling(1.0, fan_avg, uniform), biases 0.  The
    draws come from numpy.random.RandomState(seed): the reference's in distribution only."""
    rs = np.random.RandomState(seed)
    return {k: variance_scaling_uniform(rs, MCPNET_SHAPES[k]) if 'kernel' in k else np.zeros(MCPNET_SHAPES[k], np.float32) for k in NAMES}


class MCPNetTrainer(AdamTrainer):
    shapes = MCPNET_SHAPES
    names = NAMES

    def __init__(self, batch_size=BATCH_SIZE, device=None, learning_rate=1e-3, margin=1.0, beta1=0.9, beta2=0.999, epsilon=1e-8):
        if not 2 <= batch_size <= MAX_BATCH:
            raise ValueError('batch_size must be in [2, %d]' % MAX_BATCH)
        self.lib = _lib.load()
        self.dev = _device(device)
        self.B = int(batch_size)
        self.lr, self.margin = float(learning_rate), float(margin)
        self.b1, self.b2, self.eps = beta1, beta2, epsilon
        self.skipped_batches = 0

    # ---- variables ----
    def init_weights(self, seed=0):
        return self.load_weights(initial_weights(seed))

    def load_weights(self, weights):
        """weights: name -> array of the eight mcp_* trainables in the TF shapes.  Resets the optimiser (slots zero, step 0)."""
        for k, shp in MCPNET_SHAPES.items():
            if k not in weights:
                raise KeyError('MCPNet weight %s missing' % k)
            if tuple(np.shape(weights[k])) != shp:
                raise ValueError('%s has shape %s, MCPNet needs %s' % (k, np.shape(weights[k]), shp))
        B, R, H, E = self.B, self.B * NUM_NEIGHBORS, HIDDEN, EMBEDDING_SIZE
        with torch.cuda.device(self.dev):
            self._bind(weights)

            def buf(*shape, dtype=torch.float32):
                return torch.zeros(shape, dtype=dtype, device=self.dev)
            self.packed = buf(self.lib.lrg_mcp_packed_floats())
            self._x, self._c, self._labels = buf(R, 6), buf(B, 4), buf(B, dtype=torch.int32)
            self._h1, self._h2, self._cat, self._fc3, self._fc4, self._emb = buf(R, H), buf(R, H), buf(B, H + 4), buf(B, H), buf(B, E), buf(B, E)
            self._D, self._dD, self._dfc4 = buf(B, B), buf(B, B), buf(B, E)
            self._stats = buf(4, dtype=torch.float64)
            self._ws = buf(self.lib.lrg_mcp_triplet_workspace_doubles(B), dtype=torch.float64)
            self._dz3, self._dcat, self._dz2, self._dz1 = buf(B, H), buf(B, H + 4), buf(R, H), buf(R, H)
            self._cs_part = buf(B, H)
            self._dw_part = buf(max(self._dw_planes(K, N, rows)[1] * K * N for K, N, rows in ((6, H, R), (H, H, R), (H + 4, H, B), (H, E, B))))
        return self

    def weights_numpy(self):
        with torch.cuda.device(self.dev):
            return super().weights_numpy()

    def checkpoint_numpy(self):
        """Everything the reference's ``Saver`` (train_mcpnet.py:162, :227) stores: checkpoint.mcpnet_checkpoint_tensors."""
        with torch.cuda.device(self.dev):
            m, v = self.slots_numpy()
            return checkpoint.mcpnet_checkpoint_tensors(super().weights_numpy(), m, v, self.step, self.b1, self.b2)

    def save(self, prefix):
        checkpoint.write_bundle(prefix, self.checkpoint_numpy())

    # ---- the reductions over the rows (no atomics: the planes and the segments are added in ascending order) ----
    def _dw_planes(self, K, N, R):
        tiles = -(-K // 64) * -(-N // 64)
        split = max(1, min(R // 256, -(-DW_WORKGROUPS // tiles)))
        return split, self.lib.lrg_gemm_f32_planes_count(R, split)

    def _dW(self, X, dZ, K, N, R, out):
        """out[K,N] = X[R,K]^T dZ[R,N]."""
        split, planes = self._dw_planes(K, N, R)
        _lib.check(self.lib.lrg_gemm_f32_planes(K, N, R, _ptr(X), K, 1, _ptr(dZ), N, 0, _ptr(self._dw_part), split, _stream()), 'lrg_gemm_f32_planes')
        _lib.check(self.lib.lrg_segment_colsum(_ptr(self._dw_part), 1, planes, K * N, _ptr(out), _stream()), 'lrg_segment_colsum')

    def _colsum(self, x, N, rows_each, out):
        """out[N] = the column sums of x [B * rows_each, N]: per point in ascending row order, then over the points."""
        src = x
        if rows_each > 1:
            _lib.check(self.lib.lrg_segment_colsum(_ptr(x), self.B, rows_each, N, _ptr(self._cs_part), _stream()), 'lrg_segment_colsum')
            src = self._cs_part
        _lib.check(self.lib.lrg_segment_colsum(_ptr(src), 1, self.B, N, _ptr(out), _stream()), 'lrg_segment_colsum')

    def _dX(self, dZ, W, M, N, K, out, mask=None):
        """out[M,N] = dZ[M,K] W[N,K]^T, zero where mask <= 0."""
        _lib.check(self.lib.lrg_gemm_f32(M, N, K, _ptr(dZ), K, 0, _ptr(W), K, 1, _ptr(out), N, None, _ptr(mask), 1, _stream()), 'lrg_gemm_f32')

    # ---- forward and loss ----
    def _repack(self):
        v = self.views
        _lib.check(self.lib.lrg_mcp_pack_weights(*[_ptr(v[k]) for k in NAMES], _ptr(self.packed), _stream()), 'lrg_mcp_pack_weights')

    def _loss(self, fc4, emb, labels, n, D, dD, dfc4, stats, ws):
        _lib.check(self.lib.lrg_mcp_triplet_semihard(_ptr(fc4), _ptr(emb), _ptr(labels), n, ctypes.c_float(self.margin), _ptr(D), _ptr(dD),
                                                     _ptr(dfc4), _ptr(stats), _ptr(ws), _stream()), 'lrg_mcp_triplet_semihard')

    @staticmethod
    def _scalars(stats, emb):
        s = stats.cpu().numpy()
        with np.errstate(all='ignore'):
            loss = float(np.float64(s[0]) / np.float64(s[1])) if s[1] else float('nan')
        return dict(loss=loss, emb=emb.cpu().numpy(), num_positives=int(s[1]), active_pairs=int(s[2]), inside_pairs=int(s[3]))

    def _check_batch(self, points4, rows, labels, n=None):
        points4 = np.ascontiguousarray(points4, dtype=np.float32)
        n = len(points4) if n is None else n
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        labels = np.ascontiguousarray(np.asarray(labels).astype(np.int32))
        if points4.shape != (n, 4) or rows.shape != (n, NUM_NEIGHBORS, 6) or labels.shape != (n,):
            raise ValueError('a batch is points [%d, 4], rows [%d, %d, 6] and labels [%d]' % (n, n, NUM_NEIGHBORS, n))
        return points4, rows, labels

    def forward_backward(self, points4, rows, labels, mark=None):
        """The step without the update: the gradients are left in gviews.  Returns the scalars' device buffer.  mark(name), if given,
        is called after each stage (forward, loss, head_backward, branch_backward): tools/mcpnet_train_bench.py records events."""
        mark = mark or (lambda name: None)
        points4, rows, labels = self._check_batch(points4, rows, labels, self.B)
        B, R, H, E = self.B, self.B * NUM_NEIGHBORS, HIDDEN, EMBEDDING_SIZE
        v, g = self.views, self.gviews
        self._x.copy_(torch.from_numpy(rows).view(R, 6))
        self._c.copy_(torch.from_numpy(points4))
        self._labels.copy_(torch.from_numpy(labels))
        self._repack()
        _lib.check(self.lib.lrg_mcp_embed_train(_ptr(self._x), _ptr(self._c), B, _ptr(self.packed), _ptr(self._h1), _ptr(self._h2), _ptr(self._cat),
                                                _ptr(self._fc3), _ptr(self._fc4), _ptr(self._emb), _stream()), 'lrg_mcp_embed_train')
        mark('forward')
        self._loss(self._fc4, self._emb, self._labels, B, self._D, self._dD, self._dfc4, self._stats, self._ws)
        mark('loss')
        # fc4 = fc3 K4 + b4 (learn_region_grow_util.py:223-224)
        self._dW(self._fc3, self._dfc4, H, E, B, g['mcp_kernel4'])
        self._colsum(self._dfc4, E, 1, g['mcp_bias4'])
        self._dX(self._dfc4, v['mcp_kernel4'], B, H, E, self._dz3, mask=self._fc3)
        # fc3 = relu(concat K3 + b3) (:220-222)
        self._dW(self._cat, self._dz3, H + 4, H, B, g['mcp_kernel3'])
        self._colsum(self._dz3, H, 1, g['mcp_bias3'])
        self._dX(self._dz3, v['mcp_kernel3'], B, H + 4, H, self._dcat)
        mark('head_backward')
        # the max over the 50 rows and layer 2's ReLU (:215-216): equal shares among the rows that tie
        _lib.check(self.lib.lrg_pool_backward(_ptr(self._h2), ctypes.c_void_p(self._dcat.data_ptr() + 16), B, NUM_NEIGHBORS, H, H + 4, _ptr(self._dz2),
                                              _stream()), 'lrg_pool_backward')
        self._dW(self._h1, self._dz2, H, H, R, g['mcp_kernel2'])
        self._colsum(self._dz2, H, NUM_NEIGHBORS, g['mcp_bias2'])
        self._dX(self._dz2, v['mcp_kernel2'], R, H, H, self._dz1, mask=self._h1)
        # layer 1 (:210-212)
        self._dW(self._x, self._dz1, 6, H, R, g['mcp_kernel1'])
        self._colsum(self._dz1, H, NUM_NEIGHBORS, g['mcp_bias1'])
        mark('branch_backward')
        return self._stats

    def train_step(self, points4, rows, labels, mark=None):
        """sess.run([net.train_op, net.loss, net.embeddings], ...) of train_mcpnet.py:197 for a batch of B points: points4 [B, 4]
        (z, r, g, b), rows [B, 50, 6], labels [B].  dict(loss, emb [B, 10] float32, num_positives, active_pairs, inside_pairs)."""
        with torch.cuda.device(self.dev):
            out = self._scalars(self.forward_backward(points4, rows, labels, mark), self._emb)
            if out['num_positives'] == 0:
                self.skipped_batches += 1
                return out
            self._adam_update(self.lr)
            if mark:
                mark('update')
        return out

    def evaluate(self, points4, rows, labels):
        """sess.run([net.loss, net.embeddings], ...) of :217 on the current weights: any 2 <= n <= 1024 points, nothing kept."""
        points4, rows, labels = self._check_batch(points4, rows, labels)
        n = len(points4)
        if not 2 <= n <= MAX_BATCH:
            raise ValueError('a batch has 2 .. %d points' % MAX_BATCH)
        with torch.cuda.device(self.dev):
            x, c, lab = (torch.from_numpy(a).to(self.dev) for a in (rows, points4, labels))
            fc4 = torch.empty((n, EMBEDDING_SIZE), dtype=torch.float32, device=self.dev)
            emb, dfc4 = torch.empty_like(fc4), torch.empty_like(fc4)
            D = torch.empty((n, n), dtype=torch.float32, device=self.dev)
            dD = torch.empty_like(D)
            stats = torch.zeros(4, dtype=torch.float64, device=self.dev)
            ws = torch.zeros(self.lib.lrg_mcp_triplet_workspace_doubles(n), dtype=torch.float64, device=self.dev)
            self._repack()
            _lib.check(self.lib.lrg_mcp_embed_train(_ptr(x), _ptr(c), n, _ptr(self.packed), None, None, None, None, _ptr(fc4), _ptr(emb), _stream()),
                       'lrg_mcp_embed_train')
            self._loss(fc4, emb, lab, n, D, dD, dfc4, stats, ws)
            return self._scalars(stats, emb)


# ---- staging (train_mcpnet.py:70-150) ----
def carve_blocks(points, state):
    """:118-141: the lists of BLOCK point indices, in the script's order.  points [N >= BLOCK, >= 2] float32 (centred, equalised)."""
    xy = np.asarray(points, dtype=np.float32)[:, :2]
    available = np.ones(len(xy), dtype=bool)
    blocks = []
    for i in range(len(xy)):
        if not available[i]:
            continue
        tmp_range = LOCAL_RANGE
        while True:
            local_mask = np.sum((xy - xy[i]) ** 2, axis=1) < np.float32(tmp_range * tmp_range)       # float32 on both sides
            local_mask = np.nonzero(np.logical_and(local_mask, available))[0]
            if len(local_mask) >= BLOCK:
                break
            tmp_range *= 1.5
        local_mask = state.choice(local_mask, BLOCK, replace=False)
        blocks.append(local_mask)
        available[local_mask] = False
        if np.sum(available) < BLOCK:
            break
    return blocks


def stage_room(points, obj_id, state, device=None, info=None):
    """:80-141 for one room: raw points [M, >= 6] and their object ids -> (points [b, 512, 4], neighbor_points [b, 512, 50, 6],
    labels [b, 512]), float32 / int32.  `state` (a numpy RandomState) supplies the neighbour draws and then the blocks' draws, as
    numpy.random does in the script.  A room of fewer than 512 equalised points returns None after its neighbour draws (the script
    never leaves its `while True` there).  info: a dict that receives n_points, the room's equalised points."""
    room = mcpnet.prepare_room(points, device=device)
    pts = np.asarray(room['points'], dtype=np.float32)
    if info is not None:
        info['n_points'] = len(pts)
    nbr = mcpnet.neighbors([room], rng='legacy', state=state, device=device)[0]
    if len(pts) < BLOCK:
        return None
    obj = np.asarray(obj_id)[np.asarray(room['equalized_idx'])]
    blocks = carve_blocks(pts, state)
    sel = np.array(blocks)
    rows = pts[nbr[sel], :6] - pts[sel][:, :, None, :6]
    return pts[sel][:, :, 2:6].copy(), rows.astype(np.float32), obj[sel].astype(np.int32)


def stage_area(rooms, state, area=0, device=None, log=print):
    """rooms: (points, obj_id) pairs of one area -> the three stacked arrays of data/mcp_area%d.h5 (:145-148)."""
    out = ([], [], [])
    for room_id, (points, obj_id) in enumerate(rooms):
        info = {}
        staged = stage_room(points, obj_id, state, device=device, info=info)
        if staged is None:
            log('AREA %d room %d %d points: skipped, fewer than %d' % (area, room_id, info['n_points'], BLOCK))
            continue
        for dst, a in zip(out, staged):
            dst.append(a)
        log('AREA %d room %d %d points %d batches' % (area, room_id, info['n_points'], len(staged[0])))
    if not out[0]:
        return (np.zeros((0, BLOCK, 4), np.float32), np.zeros((0, BLOCK, NUM_NEIGHBORS, 6), np.float32), np.zeros((0, BLOCK), np.int32))
    return tuple(np.concatenate(a) for a in out)


def write_staged(path, points, neighbor_points, labels):
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    h5lite.write_file(path, dict(points=np.asarray(points, np.float32), neighbor_points=np.asarray(neighbor_points, np.float32),
                                 labels=np.asarray(labels, np.int32)))


def read_staged(path):
    f = h5lite.File(path)
    return f['points'].read(), f['neighbor_points'].read(), f['labels'].read()


# ---- batches and metrics (:26-68) ----
def even_sampling(labels, batch_size=BATCH_SIZE, samples_per_instance=SAMPLES_PER_INSTANCE, state=None):
    """get_even_sampling (:53-68): visit a random remaining instance and take 16 of its remaining points (all of them when at most 16
    remain, and the instance leaves the pool) until batch_size indices are drawn.  The script leaves three orders to Python 2's hash
    tables; here they are: the pool's keys in ascending label order, an instance's remaining points in ascending index (what choice
    draws from, and the order in which the last ones are appended), and the 16 drawn in choice's order."""
    state = np.random if state is None else state
    labels = np.asarray(labels)
    pool = {int(i): np.nonzero(labels == i)[0] for i in np.unique(labels)}
    idx = []
    while len(pool) > 0 and len(idx) < batch_size:
        k = sorted(pool)
        c = k[state.randint(len(k))]
        if len(pool[c]) > samples_per_instance:
            inliers = state.choice(pool[c], samples_per_instance, replace=False)
            idx.extend(int(i) for i in inliers)
            pool[c] = np.setdiff1d(pool[c], inliers)
        else:
            idx.extend(int(i) for i in pool[c])
            del pool[c]
    return idx[:batch_size]


def nn_accuracy(emb, lb):
    """get_acc (:26-32) in float64: the share of points whose nearest other embedding carries their label."""
    emb, lb = np.asarray(emb, dtype=np.float64), np.asarray(lb)
    correct = 0
    for i in range(len(lb)):
        order = np.argsort(np.sum((emb[i] - emb) ** 2, axis=1))
        correct += int(lb[i] == lb[order[1]])
    return 1.0 * correct / len(lb)


def anova(emb, lb):
    """get_anova (:34-51) in float64: (between_group, within_group, F)."""
    emb, lb = np.asarray(emb, dtype=np.float64), np.asarray(lb)
    lid = np.unique(lb)
    class_mean = np.array([emb[lb == i].mean(axis=0) for i in lid])
    overall_mean = emb.mean(axis=0)
    with np.errstate(all='ignore'):
        between_group = np.float64(sum(np.sum((class_mean[k] - overall_mean) ** 2) * np.sum(lb == i) for k, i in enumerate(lid))) / (len(lid) - 1)
        within_group = np.float64(sum(np.sum((emb[lb == i] - class_mean[k]) ** 2) for k, i in enumerate(lid))) / (len(lb) - len(lid))
        F = 0 if within_group == 0 else between_group / within_group
    return between_group, within_group, F
