"""NumPy restatement of the reference's PointNet2 baseline, the checker of learn_region_grow_amd.pointnet2 (a plain module the tests
import; nothing here is used by the package).

  - ``cells`` / ``cell_inputs``: benchmarks.py:281-298 as written there (a set of cell keys, a mask per cell, float64 input rows
    that the float32 placeholder then rounds).
  - ``ball_query``: tf_grouping_g.cu:3-36 in float32 without contraction (what lrg_query_ball_point computes bit for bit).
  - ``forward``: train_pointnet.py:113-202.  Everything that depends on xyz only (FPS, gather, ball query, three_nn, the
    inverse-distance weights) is float32 as the ops compute it, from tests/sampling_ref.py; the features run in ``dtype``
    (float64: the exact value the tests measure against; float32: NumPy / BLAS float32, whose distance from float64 sets the
    tests' bound).  ``mutate`` plants one fault (the tests confirm that the bound catches each).
  - ``segment``: benchmarks.py:300-306, :405-416 with a union-find, components numbered in ascending minimum index.
"""
import numpy as np

import baselines_ref
import sampling_ref as S

F32 = np.float32
NUM_POINT = 1024
NSAMPLE = 32
SA_LEVELS = ((1024, 0.1, (32, 32, 64)), (256, 0.2, (64, 64, 128)), (64, 0.4, (128, 128, 256)), (16, 0.8, (256, 256, 512)))
FP_LEVELS = ((256, 256), (256, 256), (256, 128), (128, 128, 128))


def variable_shapes(num_class, rgb_features):
    """name -> TF shape, from the text of train_pointnet.py:133-134, :161-162, :181-200."""
    c0 = 3 if rgb_features else 0
    feat = [c0, 64, 128, 256, 512]
    shapes = {}
    for lv, (_, _, mlp) in enumerate(SA_LEVELS):
        cin = 3 + feat[lv]
        for i, c in enumerate(mlp):
            shapes['layer%d/kernel%d' % (lv + 1, i)] = (1, 1, cin, c)
            shapes['layer%d/bias%d' % (lv + 1, i)] = (c,)
            cin = c
    up = 512
    for lv, mlp in enumerate(FP_LEVELS):
        cin = up + feat[3 - lv]
        for i, c in enumerate(mlp):
            shapes['fa_layer%d/kernel%d' % (lv + 1, i)] = (1, 1, cin, c)
            shapes['fa_layer%d/bias%d' % (lv + 1, i)] = (c,)
            cin = c
        up = mlp[-1]
    shapes.update({'kernel1': (1, 128, 128), 'bias1': (128,), 'kernel2': (1, 128, num_class), 'bias2': (num_class,)})
    return shapes


def random_weights(seed, num_class=13, rgb_features=False):
    """The 46 trainables at the real shapes: kernels from the reference's initialiser (VarianceScaling(1.0, fan_avg, uniform):
    uniform in +-sqrt(6 / (fan_in + fan_out))), biases uniform in +-0.1 so that ReLUs cut and biases matter."""
    rng = np.random.RandomState(seed)
    out = {}
    for name, shp in variable_shapes(num_class, rgb_features).items():
        if 'kernel' in name:
            lim = np.sqrt(6.0 / (shp[-2] + shp[-1]))
            out[name] = rng.uniform(-lim, lim, shp).astype(F32)
        else:
            out[name] = rng.uniform(-0.1, 0.1, shp).astype(F32)
    return out


def cells(points, grid_resolution):
    """-> {cell key (gx, gy): ascending point indices} (benchmarks.py:284-287)."""
    points = np.asarray(points, F32)
    grid = np.round(points[:, :2] / grid_resolution).astype(int)
    out = {}
    for g in set(tuple(g) for g in grid):
        out[(int(g[0]), int(g[1]))] = np.nonzero(np.all(grid == g, axis=1))[0]
    return out


def cell_inputs(points, grid_resolution):
    """-> {cell key: [1024, 6] float32 input rows} (benchmarks.py:288-295; a cell of more than 1024 points fails as :298 does)."""
    points = np.asarray(points, F32)
    out = {}
    for g, idx in cells(points, grid_resolution).items():
        grid_points = points[idx, :]
        centroid_xy = np.array(g) * grid_resolution
        centroid_z = grid_points[:, 2].min()
        grid_points[:, :2] -= centroid_xy
        grid_points[:, 2] -= centroid_z
        input_points = np.zeros((NUM_POINT, 6))
        input_points[:len(grid_points), :] = grid_points[:NUM_POINT, :6]
        input_points[len(grid_points):, :] = grid_points[0, :6]
        if len(grid_points) > NUM_POINT:
            raise ValueError('could not broadcast %d class values into %d points' % (NUM_POINT, len(grid_points)))
        out[g] = input_points.astype(F32)
    return out


def ball_query(radius, nsample, xyz1, xyz2):
    """xyz1 (b,n,3) dataset, xyz2 (b,m,3) queries -> idx (b,m,nsample) int32: the first nsample k with
    max(sqrt(d2), 1e-20) < radius, the rest of the row the first hit, a row without hits zeros."""
    xyz1, xyz2 = np.asarray(xyz1, F32), np.asarray(xyz2, F32)
    b, m = xyz2.shape[:2]
    idx = np.zeros((b, m, nsample), np.int32)
    for bi in range(b):
        d = np.maximum(np.sqrt(S.sqdist(xyz1[bi][None, :, :], xyz2[bi][:, None, :])), F32(1e-20))
        hit = d < F32(radius)
        order = np.argsort(~hit, axis=1, kind='stable')[:, :nsample]           # the hits first, in ascending k
        if order.shape[1] < nsample:
            order = np.concatenate([order, np.repeat(order[:, :1], nsample - order.shape[1], axis=1)], axis=1)
        cnt = hit.sum(axis=1)
        row = np.where(np.arange(nsample)[None, :] < cnt[:, None], order, order[:, :1])
        idx[bi] = np.where(cnt[:, None] > 0, row, 0)
    return idx


def _mlp(x, weights, scope, ids, dtype, mutate, relu_last=True):
    for n, i in enumerate(ids):
        kname, bname = '%skernel%d' % (scope, i), '%sbias%d' % (scope, i)
        w = weights[kname].reshape(weights[kname].shape[-2:]).astype(dtype)
        x = x @ w
        if mutate.get('drop_bias') != bname:
            x = x + weights[bname].astype(dtype)
        if (relu_last or n + 1 < len(ids)) and mutate.get('skip_relu') != bname:
            x = np.maximum(x, dtype(0))
    return x


def forward(batch, weights, dtype=np.float64, mutate=None):
    """batch [B, 1024, 6] float32 -> (logits [B, 1024, num_class] in dtype, levels) with levels = dict(sa=[4 x dict(fps, new_xyz,
    idx, features)], fp=[4 x dict(nn_idx, interpolated, features)]).

    mutate (one fault at a time): {'drop_bias': 'layer2/bias1'}, {'skip_relu': 'fa_layer3/bias0'} (the ReLU after that bias),
    {'dup_sample': level} (sample 31's row used twice: in place of sample 30 too), {'shift_skip': fp_level} (the skip features of
    that feature-propagation level rolled by one channel)."""
    mutate = mutate or {}
    dtype = np.dtype(dtype).type
    batch = np.asarray(batch, F32)
    rgb = weights['layer1/kernel0'].shape[2] == 6
    B = batch.shape[0]
    rows = np.arange(B)[:, None]
    xyz = [np.ascontiguousarray(batch[:, :, :3])]
    feat = [batch[:, :, 3:].astype(dtype) if rgb else None]
    levels = dict(sa=[], fp=[])
    for lv, (npoint, radius, mlp) in enumerate(SA_LEVELS):
        fps = S.farthest_point_sample(npoint, xyz[lv])
        new_xyz = S.gather_point(xyz[lv], fps)
        idx = ball_query(radius, NSAMPLE, xyz[lv], new_xyz)
        use = idx
        if mutate.get('dup_sample') == lv + 1:
            use = idx.copy()
            use[:, :, 30] = use[:, :, 31]
        grouped = (xyz[lv][rows[:, :, None], use] - new_xyz[:, :, None, :]).astype(dtype)       # float32 subtraction, then widened
        if feat[lv] is not None:
            grouped = np.concatenate([grouped, feat[lv][rows[:, :, None], use]], axis=-1)
        x = _mlp(grouped, weights, 'layer%d/' % (lv + 1), range(3), dtype, mutate)
        new_feat = x.max(axis=2)
        xyz.append(new_xyz)
        feat.append(new_feat)
        levels['sa'].append(dict(fps=fps, new_xyz=new_xyz, idx=idx, features=new_feat))
    up = feat[4]
    for lv, mlp in enumerate(FP_LEVELS):
        dst = 3 - lv
        dist, nn_idx = S.three_nn(xyz[dst], xyz[dst + 1])
        w = S.fp_weights(dist)
        if dtype is F32:
            interp = S.three_interpolate(up, nn_idx, w)
        else:
            p = [up[rows, nn_idx[:, :, u]] for u in range(3)]
            interp = (p[0] * w[:, :, 0:1].astype(dtype) + p[1] * w[:, :, 1:2].astype(dtype)) + p[2] * w[:, :, 2:3].astype(dtype)
        x = interp
        if feat[dst] is not None:
            skip = feat[dst]
            if mutate.get('shift_skip') == lv + 1:
                skip = np.roll(skip, 1, axis=2)
            x = np.concatenate([interp, skip], axis=2)
        up = _mlp(x, weights, 'fa_layer%d/' % (lv + 1), range(len(mlp)), dtype, mutate)
        levels['fp'].append(dict(nn_idx=nn_idx, interpolated=interp, features=up))
    logits = _mlp(up, weights, '', (1, 2), dtype, mutate, relu_last=False)
    return logits, levels


def classify(points, weights, grid_resolution, dtype=np.float64):
    """class_labels of one room (benchmarks.py:282-298) and the top-two logit gap of every point."""
    points = np.asarray(points, F32)
    cls = np.zeros(len(points), np.int64)
    gap = np.zeros(len(points))
    members = cells(points, grid_resolution)
    inputs = cell_inputs(points, grid_resolution)
    keys = sorted(members)
    logits, _ = forward(np.stack([inputs[k] for k in keys]), weights, dtype)
    for c, k in enumerate(keys):
        idx = members[k]
        lg = logits[c, :len(idx)]
        cls[idx] = lg.argmax(axis=1)
        top = np.sort(lg, axis=1)
        gap[idx] = top[:, -1] - top[:, -2]
    return cls, gap


def segment(points, classes, resolution=0.1, min_cluster_size=10):
    """cluster_label of one room: edges between 26-neighbour voxels of equal class, components of more than min_cluster_size points
    numbered from 1 in ascending minimum index (networkx's order for these edge lists, as tests/baselines_ref.py)."""
    points = np.asarray(points, F32)
    classes = np.asarray(classes)
    n = len(points)
    nb = baselines_ref.neighbours(points, resolution)
    ii, oo = np.nonzero(nb >= 0)
    kk = nb[ii, oo]
    sel = kk < ii
    ii, kk = ii[sel], kk[sel]
    e = classes[kk] == classes[ii]
    root = baselines_ref._roots(n, ii[e], kk[e])
    size = np.bincount(root, minlength=n)
    kept = np.nonzero((size > min_cluster_size) & (np.arange(n) == root))[0]
    ids = np.zeros(n, dtype=np.int64)
    ids[kept] = np.arange(1, len(kept) + 1)
    return ids[root]


def equalize(points, resolution=0.1):
    """(points, equalized_idx, unequalized_idx) of benchmarks.py:199-215: the first point of every round(xyz / 0.1) voxel, in
    order of first appearance."""
    points = np.asarray(points, F32)
    v = np.round(points[:, :3] / F32(resolution)).astype(np.int64)
    _, first, inv = np.unique(v, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind='stable')
    rank = np.empty(len(first), dtype=np.int64)
    rank[order] = np.arange(len(first))
    eq = first[order]
    return points[eq], eq, rank[np.asarray(inv).reshape(-1)]


def random_layers(rng, widths):
    """[(w [k, n], bias [n])] for widths = (k, n1, n2, ...): the initialiser of random_weights."""
    out = []
    for k, n in zip(widths[:-1], widths[1:]):
        lim = np.sqrt(6.0 / (k + n))
        out.append((rng.uniform(-lim, lim, (k, n)).astype(F32), rng.uniform(-0.1, 0.1, n).astype(F32)))
    return out


def row_mlp(a, b, layers, relu_last=True, dtype=np.float64):
    """concat(a, b) (b may be None) through the layers x W + bias, ReLU after each (the last only with relu_last)."""
    dtype = np.dtype(dtype).type
    x = np.asarray(a, F32).astype(dtype)
    if b is not None:
        x = np.concatenate([x, np.asarray(b, F32).astype(dtype)], axis=-1)
    for n, (w, bias) in enumerate(layers):
        x = x @ w.astype(dtype) + bias.astype(dtype)
        if relu_last or n + 1 < len(layers):
            x = np.maximum(x, dtype(0))
    return x


def group_mlp(xyz, new_xyz, points, idx, layers, dtype=np.float64):
    """A set-abstraction level after its ball query: rows concat(xyz[idx] - new_xyz (float32), points[idx]), the layers with ReLU,
    the maximum over the samples.  xyz (b,n,3), new_xyz (b,m,3), points (b,n,c) or None, idx (b,m,ns) -> (b,m,c_out)."""
    dtype = np.dtype(dtype).type
    xyz, new_xyz = np.asarray(xyz, F32), np.asarray(new_xyz, F32)
    rows = np.arange(xyz.shape[0])[:, None, None]
    g = xyz[rows, idx] - new_xyz[:, :, None, :]
    return row_mlp(g, None if points is None else np.asarray(points, F32)[rows, idx], layers, True, dtype).max(axis=2)
