"""NumPy restatement of one training step of the reference's PointNet2 (train_pointnet.py:113-211), the checker of
learn_region_grow_amd.pointnet2_train (a plain module the tests import; nothing here is used by the package).  It stands on
tests/pointnet2_ref.py (the float32 index computations, the level table) and tests/sampling_ref.py.

  - ``level_indices``: everything that depends on xyz only -- FPS, the ball queries, three_nn and the inverse-distance weights -- in
    float32 as the ops compute it; dict(sa=[dict(fps, idx)], fp=[dict(nn_idx, weight)]), the shape of
    ``PointNet2Trainer.level_indices()``, so that the device's own can be fed in instead.
  - ``forward``: :170-207 in ``dtype`` (float64: the value the tests measure against; float32: whose distance from float64 sets the
    tests' bound) ON GIVEN INDICES, with every layer kept.
  - ``backward``: the gradient of class_loss for every trainable, written out by hand (finite differences check it in
    tests/test_pointnet2_train_host.py).  Only the features carry gradients.  ``tf.reduce_max`` shares a gradient equally among the
    rows that tie for the maximum (zero where the maximum is 0: the ReLU below it); group_point's and three_interpolate's gradients
    are ``np.add.at`` scatters.
  - ``adam_update`` / ``train``: AdamOptimizer(0.001) (:210).

The widths are read from the weights and the level table is an argument, so that the gradients can be checked on small cells and
narrow layers.
"""
import numpy as np

import pointnet2_ref as P2
import sampling_ref as S

F32 = np.float32
NSAMPLE = P2.NSAMPLE
SA_LEVELS = tuple((m, r) for m, r, _ in P2.SA_LEVELS)          # (npoint, radius)


def trainable_names(weights):
    return sorted(weights)


def _layers(weights, scope, ids):
    return [(weights['%skernel%d' % (scope, i)], weights['%sbias%d' % (scope, i)], '%skernel%d' % (scope, i), '%sbias%d' % (scope, i)) for i in ids]


def _fp_ids(weights, lv):
    n = 0
    while 'fa_layer%d/kernel%d' % (lv + 1, n) in weights:
        n += 1
    return range(n)


def level_indices(batch, sa_levels=SA_LEVELS):
    batch = np.asarray(batch, F32)
    xyz = [np.ascontiguousarray(batch[:, :, :3])]
    out = dict(sa=[], fp=[])
    for npoint, radius in sa_levels:
        fps = S.farthest_point_sample(npoint, xyz[-1])
        new_xyz = S.gather_point(xyz[-1], fps)
        out['sa'].append(dict(fps=fps, idx=P2.ball_query(radius, NSAMPLE, xyz[-1], new_xyz)))
        xyz.append(new_xyz)
    for lv in range(len(sa_levels)):
        dst = len(sa_levels) - 1 - lv
        dist, nn_idx = S.three_nn(xyz[dst], xyz[dst + 1])
        out['fp'].append(dict(nn_idx=nn_idx, weight=S.fp_weights(dist)))
    return out


def _mlp(x, layers, dtype, relu_last=True):
    """-> the layers' outputs (post-ReLU)"""
    acts = []
    for n, (w, b, _, _) in enumerate(layers):
        x = (x.reshape(-1, x.shape[-1]) @ w.reshape(w.shape[-2:]).astype(dtype)).reshape(x.shape[:-1] + (w.shape[-1],)) + b.astype(dtype)    # one 2-D product
        if relu_last or n + 1 < len(layers):
            x = np.maximum(x, dtype(0))
        acts.append(x)
    return acts


def forward(batch, labels, weights, ind, dtype=np.float64):
    """batch [B, n, 6] float32, labels [B, n], ind as level_indices -> dict(loss, acc, logits and what backward needs)."""
    dtype = np.dtype(dtype).type
    batch = np.asarray(batch, F32)
    rgb = weights['layer1/kernel0'].shape[2] == 6
    B, L = batch.shape[0], len(ind['sa'])
    rows = np.arange(B)[:, None]
    xyz = [np.ascontiguousarray(batch[:, :, :3])]
    feat = [batch[:, :, 3:].astype(dtype) if rgb else None]
    sa, fp = [], []
    for lv in range(L):
        fps, idx = ind['sa'][lv]['fps'], ind['sa'][lv]['idx']
        new_xyz = S.gather_point(xyz[lv], fps)
        grouped = (xyz[lv][rows[:, :, None], idx] - new_xyz[:, :, None, :]).astype(dtype)       # float32 subtraction, then widened
        if feat[lv] is not None:
            grouped = np.concatenate([grouped, feat[lv][rows[:, :, None], idx]], axis=-1)
        acts = _mlp(grouped, _layers(weights, 'layer%d/' % (lv + 1), range(3)), dtype)
        xyz.append(new_xyz)
        feat.append(acts[-1].max(axis=2))
        sa.append(dict(rows=grouped, acts=acts, idx=idx))
    up = feat[L]
    for lv in range(L):
        dst = L - 1 - lv
        nn_idx, w = ind['fp'][lv]['nn_idx'], np.asarray(ind['fp'][lv]['weight'], F32).astype(dtype)
        p = [up[rows, nn_idx[:, :, u]] for u in range(3)]
        interp = (p[0] * w[:, :, 0:1] + p[1] * w[:, :, 1:2]) + p[2] * w[:, :, 2:3]
        x = interp if feat[dst] is None else np.concatenate([interp, feat[dst]], axis=2)
        acts = _mlp(x, _layers(weights, 'fa_layer%d/' % (lv + 1), _fp_ids(weights, lv)), dtype)
        fp.append(dict(x=x, acts=acts, nn_idx=nn_idx, weight=w, c_up=interp.shape[2], interpolated=interp))
        up = acts[-1]
    head = _mlp(up, _layers(weights, '', (1, 2)), dtype, relu_last=False)
    logits = head[-1]
    lab = np.asarray(labels).astype(np.int64)
    m = logits.max(axis=2, keepdims=True)
    lse = np.log(np.exp(logits - m).sum(axis=2)) + m[..., 0]
    picked = np.take_along_axis(logits, lab[..., None], axis=2)[..., 0]
    return dict(loss=float((lse - picked).mean()), acc=float((logits.argmax(axis=2) == lab).mean()), logits=logits, labels=lab, sa=sa, fp=fp,
                head_in=up, fc1=head[0], feat=feat, rgb=rgb)


def _mlp_backward(g, x, acts, layers, dz, dtype, need_dx=True):
    """dz: the gradient of the last layer's pre-activation.  Fills g for the layers; -> the gradient of x (None unless need_dx)."""
    for i in range(len(layers) - 1, -1, -1):
        w, _, kname, bname = layers[i]
        inp = x if i == 0 else acts[i - 1]
        k = inp.shape[-1]
        g[kname] = (inp.reshape(-1, k).T @ dz.reshape(-1, dz.shape[-1])).reshape(w.shape)
        g[bname] = dz.reshape(-1, dz.shape[-1]).sum(axis=0)
        if i == 0 and not need_dx:
            return None
        dx = (dz.reshape(-1, dz.shape[-1]) @ w.reshape(w.shape[-2:]).astype(dtype).T).reshape(dz.shape[:-1] + (k,))
        if i > 0:
            dz = np.where(inp > 0, dx, dtype(0))
    return dx


def backward(fw, weights, dtype=np.float64):
    """d class_loss / d every trainable (TF shapes), from forward()'s record."""
    dtype = np.dtype(dtype).type
    logits, lab = fw['logits'], fw['labels']
    B, n0 = lab.shape
    L = len(fw['sa'])
    rows = np.arange(B)[:, None]
    g = {}
    m = logits.max(axis=2, keepdims=True)
    e = np.exp(logits - m)
    d = e / e.sum(axis=2, keepdims=True)
    np.put_along_axis(d, lab[..., None], np.take_along_axis(d, lab[..., None], axis=2) - dtype(1), axis=2)
    d = d / dtype(B * n0)
    dup = _mlp_backward(g, fw['head_in'], [fw['fc1'], logits], _layers(weights, '', (1, 2)), d, dtype)
    dfeat = [None] * (L + 1)
    for lv in range(L - 1, -1, -1):
        rec, dst = fw['fp'][lv], L - 1 - lv
        dz = np.where(rec['acts'][-1] > 0, dup, dtype(0))
        dx = _mlp_backward(g, rec['x'], rec['acts'], _layers(weights, 'fa_layer%d/' % (lv + 1), _fp_ids(weights, lv)), dz, dtype)
        c_up = rec['c_up']
        if dst >= 1:
            dfeat[dst] = dx[..., c_up:].copy()                                            # the skip connection: the first contributor
        msrc = fw['feat'][dst + 1].shape[1]
        nq = dx.shape[1]
        vals = (dx[:, :, None, :c_up] * rec['weight'][:, :, :, None]).reshape(B, nq * 3, c_up)      # entry e = 3 * query + u
        dsrc = np.zeros((B, msrc, c_up), dtype)
        np.add.at(dsrc, (rows, rec['nn_idx'].reshape(B, nq * 3)), vals)
        if lv > 0:
            dup = dsrc
        else:
            dfeat[L] = dsrc
    for lv in range(L - 1, -1, -1):
        rec = fw['sa'][lv]
        y = rec['acts'][-1]                                                               # [B, m, 32, w3]
        mx = y.max(axis=2, keepdims=True)
        tie = y == mx
        share = dfeat[lv + 1][:, :, None, :] / tie.sum(axis=2, keepdims=True).astype(dtype)
        dz = np.where(tie & (mx > 0), share, dtype(0))
        dx = _mlp_backward(g, rec['rows'], rec['acts'], _layers(weights, 'layer%d/' % (lv + 1), range(3)), dz, dtype, need_dx=lv >= 1)
        if lv >= 1:
            c = dx.shape[-1] - 3
            np.add.at(dfeat[lv], (rows, rec['idx'].reshape(B, -1)), dx[..., 3:].reshape(B, -1, c))
    return g


def loss_and_grads(batch, labels, weights, ind=None, dtype=np.float64):
    fw = forward(batch, labels, weights, level_indices(batch) if ind is None else ind, dtype)
    return fw, backward(fw, weights, dtype)


def adam_update(p, g, m, v, step, lr=0.001, beta1=0.9, beta2=0.999, epsilon=1e-8, dtype=np.float64):
    """One AdamOptimizer(0.001) update at global step `step` (0 for the first): returns (p, m, v)."""
    t = step + 1
    lr_t = lr * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
    p, g, m, v = (np.asarray(a, dtype) for a in (p, g, m, v))
    m = m + (g - m) * dtype(1 - beta1)
    v = v + (g * g - v) * dtype(1 - beta2)
    return p - dtype(lr_t) * m / (np.sqrt(v) + dtype(epsilon)), m, v


def train(batches, weights, dtype=np.float64, **adam):
    """The reference's loop on the batches [(points, labels, indices or None)]: returns (weights, [loss per step])."""
    w = {k: np.asarray(a).astype(dtype) for k, a in weights.items()}
    m = {k: np.zeros_like(w[k]) for k in w}
    v = {k: np.zeros_like(w[k]) for k in w}
    losses = []
    for step, (pts, lab, ind) in enumerate(batches):
        fw, g = loss_and_grads(pts, lab, w, ind, dtype)
        losses.append(fw['loss'])
        for k in w:
            w[k], m[k], v[k] = adam_update(w[k], g[k], m[k], v[k], step, dtype=dtype, **adam)
    return w, losses
