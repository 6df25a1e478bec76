"""NumPy restatement of the benchmarks.py baselines (modes normal, curvature, color, feature, smoothness; benchmarks.py:251-416).

Features come from ``features`` (benchmarks.py:199-249 through learn_region_grow_amd.preprocess's host covariances and the
reference's own ``numpy.linalg.svd``).  The edge predicates are restated without ``numpy.dot``, whose rounding depends on the
CPU's BLAS kernel:
  normal      fma(a2, b2, fma(a1, b1, a0 * b0)) > t  (OpenBLAS ddot for n = 3).  Evaluated as the plain float64 sum and, where that
              lies within 1e-12 of t (the two differ by a few ulps), again through libm's fma by ctypes.
  curvature   |c_k - c_i| < t in float64
  color       float32 squares summed (d0 + d1) + d2, compared with float32(t)
Components by union-find; numbering by the smallest point index (networkx's order) or, for smoothness, the smallest argsort rank;
smoothness components of 2 .. min_cluster_size points are decided by the literal DFS of :384-405, whose pop count counts duplicates.
"""
import ctypes
import ctypes.util
import hashlib
import itertools
import sys

import numpy as np

from learn_region_grow_amd import preprocess, synthetic

_libm = ctypes.CDLL(ctypes.util.find_library('m'))
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double] * 3
OFFSETS = [o for o in itertools.product([-1, 0, 1], [-1, 0, 1], [-1, 0, 1]) if o != (0, 0, 0)]
VOX_OFF = 1 << 20


def sparse_patch_room(seed=11, n_patches=120):
    """Axis-aligned planar patches of 1 x 1 .. 4 x 3 voxels (3 raw points a voxel) scattered over a 12 x 12 x 3 m box: many small
    smoothness regions, some kept only because the reference counts duplicate pops."""
    rs = np.random.RandomState(seed)
    rows = []
    for j in range(n_patches):
        a, b = rs.randint(1, 5), rs.randint(1, 4)
        axis = rs.randint(3)
        base = np.round(rs.uniform([0, 0, 0], [120, 120, 30])).astype(int)
        color = rs.uniform(0, 1, 3)
        for u in range(a):
            for v in range(b):
                cell = base.copy()
                cell[(axis + 1) % 3] += u
                cell[(axis + 2) % 3] += v
                for _ in range(3):
                    p = cell * 0.1 + rs.uniform(-0.03, 0.03, 3)
                    p[axis] = cell[axis] * 0.1 + rs.normal(0, 0.002)
                    rows.append(np.concatenate([p, np.clip(color + rs.normal(0, 0.01, 3), 0, 1), [j + 1, 1]]))
    return np.array(rows, dtype=np.float32)


def golden_rooms():
    """The three raw rooms of tests/golden/baselines_ref_cpu.npz (x, y, z, r, g, b, object id, class id), regenerated from their
    seeds; the golden pins them by rooms_digest."""
    return [synthetic.generate_room_points(40000, 7).astype(np.float32),
            synthetic.generate_room_points(40000, 8).astype(np.float32),
            sparse_patch_room()]


def rooms_digest(rooms):
    h = hashlib.sha256()
    for r in rooms:
        h.update(np.ascontiguousarray(r, dtype=np.float32).tobytes())
    return h.hexdigest()


def fma(a, b, c):
    return _libm.fma(float(a), float(b), float(c))


def ddot3(a, b):
    """OpenBLAS ddot of two float64 3-vectors: fma(a2, b2, fma(a1, b1, a0 * b0))."""
    return fma(a[2], b[2], fma(a[1], b[1], float(a[0]) * float(b[0])))


def features(unequalized_points, resolution=0.1):
    """benchmarks.py:199-249: equalised float32 xyzrgb, |V[2]| and |S[2] / sum(S)| in float64 (not normalised), argsort ranks."""
    raw = np.asarray(unequalized_points, dtype=np.float32)
    p = preprocess.preprocess_room(raw[:, :6], np.zeros(len(raw), int), np.zeros(len(raw), int), resolution=resolution, return_cov=True)
    _, S, V = np.linalg.svd(p['cov'])
    c = np.fabs(S[:, 2] / (S[:, 0] + S[:, 1] + S[:, 2]))
    rank = np.empty(len(c), dtype=np.int32)
    rank[np.argsort(c)] = np.arange(len(c), dtype=np.int32)
    return dict(points=raw[p['equalized_idx'], :6], normals=np.fabs(V[:, 2, :]), curvatures=c, rank=rank,
                equalized_idx=p['equalized_idx'], unequalized_idx=p['unequalized_idx'])


def neighbours(points, resolution):
    """[N, 26] index of the point in each neighbouring voxel (offsets in itertools.product order), -1 where empty."""
    v = np.round(points[:, :3] / np.float32(resolution)).astype(np.int64)        # :254-256, float32 / float32
    key = lambda w: ((w[:, 0] + VOX_OFF) << 42) | ((w[:, 1] + VOX_OFF) << 21) | (w[:, 2] + VOX_OFF)
    k = key(v)
    order = np.argsort(k, kind='stable')
    sk = k[order]
    if len(sk) > 1 and (np.diff(sk) == 0).any():
        raise ValueError('two points share a voxel: the room is not equalised')
    nb = np.full((len(points), 26), -1, dtype=np.int64)
    for o, off in enumerate(OFFSETS):
        q = key(v + np.array(off))
        pos = np.minimum(np.searchsorted(sk, q), max(len(sk) - 1, 0))
        hit = sk[pos] == q if len(sk) else np.zeros(0, bool)
        nb[hit, o] = order[pos[hit]]
    return nb


def normal_edge(normals, i, k, t):
    """normals[k].dot(normals[i]) > t for index arrays i, k."""
    a, b = normals[k], normals[i]
    plain = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
    out = plain > t
    for j in np.nonzero(np.abs(plain - t) <= 1e-12)[0]:
        out[j] = ddot3(a[j], b[j]) > t
    return out


def curvature_edge(curv, i, k, t):
    return np.abs(curv[k] - curv[i]) < t


def color_edge(points, i, k, t):
    d = (points[k, 3:6] - points[i, 3:6]).astype(np.float32)
    sq = d * d
    s = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
    return s < np.float32(t)


def edge_mask(room, mode, t, i, k):
    if mode in ('normal', 'smoothness'):
        return normal_edge(room['normals'], i, k, t[0])
    if mode == 'curvature':
        return curvature_edge(room['curvatures'], i, k, t[0])
    if mode == 'color':
        return color_edge(room['points'], i, k, t[0])
    if mode == 'feature':
        return normal_edge(room['normals'], i, k, t[0]) & curvature_edge(room['curvatures'], i, k, t[1]) & \
            color_edge(room['points'], i, k, t[2])
    raise ValueError(mode)


def _roots(n, ei, ek):
    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in zip(ei.tolist(), ek.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)             # the root of a component is its minimum index
    return np.array([find(x) for x in range(n)], dtype=np.int64)


def dfs_pops(nb, normals, t, seed, visited):
    """The literal DFS of :384-405 from seed; marks visited, returns C (with duplicates)."""
    Q = [seed]
    C = []
    while Q:
        i = Q.pop()
        C.append(i)
        visited[i] = True
        for k in nb[i]:
            if k >= 0 and not visited[k] and ddot3(normals[k], normals[i]) > t:
                Q.append(int(k))
    return C


def segment(room, mode, thresholds, resolution=0.1, min_cluster_size=10, distinct_only=False):
    """cluster_label of one room as benchmarks.py computes it.  distinct_only=True sizes smoothness regions by their distinct
    points instead of len(C) (what the reference does NOT do: used to show the golden depends on the difference)."""
    pts = room['points']
    n = len(pts)
    nb = neighbours(pts, resolution)
    ii, oo = np.nonzero(nb >= 0)
    kk = nb[ii, oo]
    sel = kk < ii                                                                       # every predicate is symmetric
    ii, kk = ii[sel], kk[sel]
    e = edge_mask(room, mode, thresholds, ii, kk)
    root = _roots(n, ii[e], kk[e])
    size = np.bincount(root, minlength=n)
    labels = np.zeros(n, dtype=np.int64)
    if mode != 'smoothness':
        kept = np.nonzero((size > min_cluster_size) & (np.arange(n) == root))[0]     # roots in ascending order = networkx's order
        ids = np.zeros(n, dtype=np.int64)
        ids[kept] = np.arange(1, len(kept) + 1)
        labels = ids[root]
        return labels
    rank = room['rank']
    minrank = np.full(n, n, dtype=np.int64)
    np.minimum.at(minrank, root, rank)
    roots = np.nonzero(np.arange(n) == root)[0]
    roots = roots[np.argsort(minrank[roots])]
    inv = np.empty(n, dtype=np.int64)
    inv[rank] = np.arange(n)
    visited = np.zeros(n, dtype=bool)
    ids = np.zeros(n, dtype=np.int64)
    nxt = 1
    for r in roots:
        c = size[r]
        if c > min_cluster_size:
            keep = True
        elif c < 2 or distinct_only:
            keep = c > min_cluster_size
        else:
            keep = len(dfs_pops(nb, room['normals'], thresholds[0], int(inv[minrank[r]]), visited)) > min_cluster_size
        if keep:
            ids[r] = nxt
            nxt += 1
    return ids[root]


def segment_literal_smoothness(room, threshold, resolution=0.1, min_cluster_size=10):
    """The whole of :380-405 literally (seeds in argsort order, every region by DFS): slow, for small rooms."""
    pts = room['points']
    n = len(pts)
    nb = neighbours(pts, resolution)
    labels = np.zeros(n, dtype=np.int64)
    visited = np.zeros(n, dtype=bool)
    inv = np.empty(n, dtype=np.int64)
    inv[room['rank']] = np.arange(n)
    cid = 1
    for seed in inv:
        if visited[seed]:
            continue
        C = dfs_pops(nb, room['normals'], threshold, int(seed), visited)
        if len(C) > min_cluster_size:
            labels[C] = cid
            cid += 1
    return labels


if __name__ == '__main__':
    sys.exit(__doc__)
