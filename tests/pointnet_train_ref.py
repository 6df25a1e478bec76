"""NumPy restatement of one training step of the reference's plain PointNet (train_pointnet.py:31-111, :235-246, :327-350), the
checker of learn_region_grow_amd.pointnet_train (a plain module the tests import; nothing here is used by the package).

  - ``init_like``: every trainable at its real shape in ranges that make every tensor matter (tests/pointnet_ref.random_weights),
    for any number of rows per cell.
  - ``forward``: :49-105 with ``is_training_pl: True`` in ``dtype`` (float64: the value the tests measure against; float32: whose
    distance from float64 sets the tests' bound).  The batch norm's moments run over the batch axis only (:92).
  - ``backward``: the gradient of class_loss for every trainable, written out by hand (finite differences check it in
    tests/test_pointnet_train_host.py): the batch norm in training mode with the ReLU of :93, and the gradient of the tiled max pool
    of :56-59 by the single-winner rule (the FIRST row of the cell that holds the maximum; ``tie='last'`` breaks it the other way).
  - ``ema_update``, ``learning_rate``, ``adam_update``: :71-78, :109, :110.
  - ``stage_cells``, ``jitter``: :327-350 and :235-246, line by line.

Rows per cell is whatever the inputs have (the network itself has 1024), so that the gradients can be checked cheaply.
"""
import numpy as np

import pointnet_ref

BN_EPSILON = pointnet_ref.BN_EPSILON
bn_names = pointnet_ref.bn_names


def trainable_names(conv, fc):
    """kernel*, bias*, fc_weights*, fc_bias*, and every block's beta and gamma: what tf.compat.v1.trainable_variables() holds."""
    names = []
    for i in range(len(conv)):
        names += ['kernel%d' % i, 'bias%d' % i]
    for j in range(len(fc) + 1):
        names += ['fc_weights%d' % j, 'fc_bias%d' % j]
        if j < len(fc):
            names += list(bn_names(j)[:2])
    return names


def init_like(seed, conv, fc, num_class, rows=1024):
    """Trainables from pointnet_ref.random_weights (so biases, beta and gamma are NOT at their initial 0 / 1: every term of the
    gradient is exercised); the moving averages [rows, c] zero as ExponentialMovingAverage starts them."""
    w = pointnet_ref.random_weights(seed, conv, fc, num_class)
    out = {k: w[k] for k in trainable_names(conv, fc)}
    for j, c in enumerate(fc):
        out[bn_names(j)[2]] = np.zeros((rows, c), np.float32)
        out[bn_names(j)[3]] = np.zeros((rows, c), np.float32)
    return out


def forward(points, labels, weights, dtype=np.float64):
    """points [B, P, 6], labels [B, P] -> dict(loss, acc, logits, and everything backward needs)."""
    dtype = np.dtype(dtype).type
    conv_w, fc_w, num_class = pointnet_ref.widths_of(weights)
    conv = pointnet_ref.features(points, weights, dtype)                                   # :49-54
    last = conv[-1]
    pooled = last.max(axis=1)                                                              # :56
    t = last - pooled[:, None, :]                                                          # :57-59
    h = np.concatenate([t, conv[1]], axis=2)                                               # :60-61
    B = h.shape[0]
    hs, zs, ys, means, variances = [h], [], [], [], []
    for j in range(len(fc_w)):
        z = h @ weights['fc_weights%d' % j][0].astype(dtype) + weights['fc_bias%d' % j].astype(dtype)        # :90-91
        mean = z.sum(axis=0) / dtype(B)                                                    # tf.nn.moments(axes=[0]) :70
        variance = ((z - mean) ** 2).sum(axis=0) / dtype(B)
        beta, gamma = (weights[n].astype(dtype) for n in bn_names(j)[:2])
        inv = (dtype(1) / np.sqrt(variance + dtype(BN_EPSILON))) * gamma                   # tf.nn.batch_normalization :83
        h = np.maximum(z * inv + (beta - mean * inv), dtype(0))                            # :93
        zs.append(z); ys.append(h); means.append(mean); variances.append(variance); hs.append(h)
    j = len(fc_w)
    logits = h @ weights['fc_weights%d' % j][0].astype(dtype) + weights['fc_bias%d' % j].astype(dtype)       # :98-99
    lab = np.asarray(labels).astype(np.int64)
    m = logits.max(axis=2, keepdims=True)
    lse = np.log(np.exp(logits - m).sum(axis=2)) + m[..., 0]
    picked = np.take_along_axis(logits, lab[..., None], axis=2)[..., 0]
    loss = (lse - picked).mean()                                                           # :102
    acc = float((logits.argmax(axis=2) == lab).mean())                                     # :104-105
    return dict(loss=float(loss), acc=acc, logits=logits, conv=conv, pooled=pooled, t=t, hs=hs, zs=zs, ys=ys, means=means,
                variances=variances, points=np.asarray(points, np.float32).astype(dtype), labels=lab)


def pool_winner(last, pooled, tie='first'):
    """[B, c] the row of every (cell, channel) that receives the max pool's gradient."""
    hit = last == pooled[:, None, :]
    if tie == 'first':
        return hit.argmax(axis=1)
    return last.shape[1] - 1 - hit[:, ::-1].argmax(axis=1)


def backward(fw, weights, dtype=np.float64, tie='first'):
    """d class_loss / d every trainable (TF shapes), from forward()'s record.  Also 'dz' (the hidden fc layers' pre-activation
    gradients) and 'dlast' under the key '_' for the tests that look inside."""
    dtype = np.dtype(dtype).type
    conv_w, fc_w, num_class = pointnet_ref.widths_of(weights)
    conv, lab, logits = fw['conv'], fw['labels'], fw['logits']
    B, P = lab.shape
    R = B * P
    g = {}
    m = logits.max(axis=2, keepdims=True)
    e = np.exp(logits - m)
    d = e / e.sum(axis=2, keepdims=True)
    np.put_along_axis(d, lab[..., None], np.take_along_axis(d, lab[..., None], axis=2) - dtype(1), axis=2)
    d = d / dtype(R)                                                                       # d loss / d logits
    j = len(fc_w)
    g['fc_weights%d' % j] = (fw['hs'][j].reshape(R, -1).T @ d.reshape(R, -1))[None]
    g['fc_bias%d' % j] = d.sum(axis=(0, 1))
    dh = d @ weights['fc_weights%d' % j][0].astype(dtype).T
    dzs = [None] * len(fc_w)
    for j in range(len(fc_w) - 1, -1, -1):
        z, y, mean, variance = fw['zs'][j], fw['ys'][j], fw['means'][j], fw['variances'][j]
        gamma = weights[bn_names(j)[1]].astype(dtype)
        gr = np.where(y > 0, dh, dtype(0))                                                 # the ReLU of :93
        rstd = dtype(1) / np.sqrt(variance + dtype(BN_EPSILON))
        xhat = (z - mean) * rstd
        g[bn_names(j)[0]] = gr.sum(axis=(0, 1))
        g[bn_names(j)[1]] = (gr * xhat).sum(axis=(0, 1))
        dz = gamma * rstd * (gr - gr.sum(axis=0) / dtype(B) - xhat * ((gr * xhat).sum(axis=0) / dtype(B)))
        dzs[j] = dz
        g['fc_weights%d' % j] = (fw['hs'][j].reshape(R, -1).T @ dz.reshape(R, -1))[None]
        g['fc_bias%d' % j] = dz.sum(axis=(0, 1))
        dh = dz @ weights['fc_weights%d' % j][0].astype(dtype).T
    c_last = conv_w[-1]
    dt, dskip = dh[..., :c_last], dh[..., c_last:]
    last, pooled = conv[-1], fw['pooled']
    dlast = dt.copy()
    win = pool_winner(last, pooled, tie)                                                   # [B, c]
    S = dt.sum(axis=1)
    bi, ci = np.meshgrid(np.arange(B), np.arange(c_last), indexing='ij')
    dlast[bi, win, ci] -= S
    n = len(conv_w)
    grads_act = [None] * n                                                                 # gradient of conv[i] (post-ReLU)
    grads_act[n - 1] = dlast
    grads_act[1] = dskip if grads_act[1] is None else grads_act[1] + dskip
    x = fw['points']
    for i in range(n - 1, -1, -1):
        dpre = np.where(conv[i] > 0, grads_act[i], dtype(0))
        inp = x if i == 0 else conv[i - 1]
        k = weights['kernel%d' % i]
        g['kernel%d' % i] = (inp.reshape(R, -1).T @ dpre.reshape(R, -1)).reshape(k.shape)
        g['bias%d' % i] = dpre.sum(axis=(0, 1))
        if i > 0:
            back = dpre @ k.reshape(-1, k.shape[-1]).astype(dtype).T
            grads_act[i - 1] = back if grads_act[i - 1] is None else grads_act[i - 1] + back
    g['_'] = dict(dz=dzs, dlast=dlast, winner=win)
    return g


def loss_and_grads(points, labels, weights, dtype=np.float64, tie='first'):
    fw = forward(points, labels, weights, dtype)
    return fw, backward(fw, weights, dtype, tie)


def ema_update(shadow, value, decay=0.9):
    """ExponentialMovingAverage.apply (:71-78) in float32: shadow -= (shadow - value) * (1 - decay); shadows start at 0, no debias."""
    shadow = np.asarray(shadow, np.float32)
    return shadow - (shadow - np.asarray(value, np.float32)) * np.float32(1 - decay)


def learning_rate(step, base=2e-4, decay_steps=500, decay_rate=0.5):
    """tf.compat.v1.train.exponential_decay(base, step, 500, 0.5, staircase=True) (:109)."""
    return base * decay_rate ** (step // decay_steps)


def adam_update(p, g, m, v, step, base=2e-4, decay_steps=500, decay_rate=0.5, beta1=0.9, beta2=0.999, epsilon=1e-8, dtype=np.float64):
    """One AdamOptimizer update at global step `step` (0 for the first): returns (p, m, v)."""
    t = step + 1
    lr_t = learning_rate(step, base, decay_steps, decay_rate) * np.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
    p, g, m, v = (np.asarray(a, dtype) for a in (p, g, m, v))
    m = m + (g - m) * dtype(1 - beta1)
    v = v + (g * g - v) * dtype(1 - beta2)
    return p - dtype(lr_t) * m / (np.sqrt(v) + dtype(epsilon)), m, v


def train(points_fn, weights, steps, dtype=np.float64, **adam):
    """`steps` steps of the reference's loop on the batches points_fn(step) -> (points, labels): returns (weights, [loss per step])."""
    conv_w, fc_w, _ = pointnet_ref.widths_of(weights)
    names = trainable_names(conv_w, fc_w)
    w = {k: np.asarray(a).astype(dtype) for k, a in weights.items()}
    m = {k: np.zeros_like(w[k]) for k in names}
    v = {k: np.zeros_like(w[k]) for k in names}
    losses = []
    for step in range(steps):
        pts, lab = points_fn(step)
        fw, g = loss_and_grads(pts, lab, w, dtype)
        losses.append(fw['loss'])
        for j in range(len(fc_w)):
            w[bn_names(j)[2]] = ema_update(w[bn_names(j)[2]], fw['means'][j])
            w[bn_names(j)[3]] = ema_update(w[bn_names(j)[3]], fw['variances'][j])
        for k in names:
            w[k], m[k], v[k] = adam_update(w[k], g[k], m[k], v[k], step, dtype=dtype, **adam)
    return w, losses


# ---- staging (:327-350) and jitter (:235-246), from the script line by line; rng stands for the numpy.random module ----
def stage_cells(points, cls_id, area, rng, num_point=1024):
    out_points, out_labels = [], []
    grid_resolution = 3.0 if 'kitti' in area else 1.0                                     # :331
    grid = np.round(points[:, :2] / grid_resolution).astype(int)                          # :332
    grid_set = set([tuple(g) for g in grid])                                              # :333
    for g in grid_set:                                                                    # :335
        grid_mask = np.all(grid == g, axis=1)
        grid_points = points[grid_mask, :6]
        centroid_xy = np.array(g) * grid_resolution
        centroid_z = grid_points[:, 2].min()
        grid_points[:, :2] -= centroid_xy
        grid_points[:, 2] -= centroid_z
        grid_labels = cls_id[grid_mask]
        subset = rng.choice(len(grid_points), num_point * 2, replace=len(grid_points) < num_point * 2)       # :344
        out_points.append(grid_points[subset])
        out_labels.append(grid_labels[subset])
    return np.array(out_points), np.array(out_labels)


def jitter(points, rng):
    output_points = points.copy()                                                         # :236
    for i in range(len(points)):
        if rng.randint(2):
            output_points[i, :, 0] = -output_points[i, :, 0]
        if rng.randint(2):
            output_points[i, :, 1] = -output_points[i, :, 1]
        C = rng.rand() * 0.5 + 0.75
        T = rng.rand(3) * 0.4 - 0.2
        output_points[i, :, :3] = output_points[i, :, :3] * C + T
    return output_points
