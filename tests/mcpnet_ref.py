"""NumPy restatement of test_mcpnet.py (MCPNet; network learn_region_grow_util.py:210-225), for the tests.

  center / equalize   :71-92, centring in float32 first, then the first point per round(x / 0.1) voxel
  candidates          :95-103, 27 cells round(x / 0.3) around a point's own cell (dz fastest), members ascending, itself included
  legacy_neighbors    :104 numpy.random.choice(list, 50, replace=len < 50) per point, one RandomState through every room
  counter_neighbors   the device definition on oracle/rng_ref.py's Philox and Feistel
  forward             the network in float64 (or float32), every layer returned
  edges / components  :122-145 without networkx: sequential float64 dot > t, union-find, components of more than 10 points in
                      order of their smallest index
  room_metrics        :146-170 literally (mask loops, set(obj_id) order)
  ply colours         :184-193
"""
import hashlib
import sys

import numpy as np

import baselines_ref
from learn_region_grow_amd import synthetic
from oracle import rng_ref

K = 50
PURPOSE_MCP_NEIGHBOR = 4                 # lrg_rng.h: LRG_PURPOSE_MCP_NEIGHBOR
OFFSETS27 = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]


def golden_rooms(seeds=(21, 22, 11)):
    """The three raw rooms of tests/golden/mcpnet_ref_cpu.npz (x, y, z, r, g, b, object id, class id), from their seeds: two small
    box rooms and the sparse patch room of baselines_ref."""
    return [synthetic.generate_room_points(3000, seeds[0]).astype(np.float32),
            synthetic.generate_room_points(3000, seeds[1]).astype(np.float32),
            baselines_ref.sparse_patch_room(seed=seeds[2], n_patches=60)]


def rooms_digest(rooms):
    return baselines_ref.rooms_digest(rooms)


def center(raw):
    p = np.array(np.asarray(raw)[:, :6], dtype=np.float32)
    centroid = 0.5 * (p[:, :2].min(axis=0) + p[:, :2].max(axis=0))
    p[:, :2] -= centroid
    p[:, 2] -= p[:, 2].min()
    return p


def equalize(centred, resolution=0.1):
    """(points, equalized_idx, unequalized_idx): the first point of every round(x / 0.1) voxel, in order of first appearance."""
    v = np.round(centred[:, :3] / np.float32(resolution)).astype(np.int64)
    _, first, inv = np.unique(v, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind='stable')
    rank = np.empty(len(first), dtype=np.int64)
    rank[order] = np.arange(len(first))
    eq = first[order]
    return centred[eq], eq, rank[inv.reshape(-1)]


def candidates(points, radius=0.3):
    """List of int64 arrays: the candidates of every point in the reference's order."""
    c = np.round(points[:, :3] / np.float32(radius)).astype(np.int64)
    cells = {}
    for i, key in enumerate(map(tuple, c.tolist())):
        cells.setdefault(key, []).append(i)
    out = []
    for key in map(tuple, c.tolist()):
        lst = []
        for o in OFFSETS27:
            lst.extend(cells.get((key[0] + o[0], key[1] + o[1], key[2] + o[2]), ()))
        out.append(np.array(lst, dtype=np.int64))
    return out


def legacy_neighbors(cands, state):
    return np.array([c[state.choice(len(c), K, replace=len(c) < K)] for c in cands], dtype=np.int64).reshape(-1, K)


def counter_positions(count, seed, room_id, point):
    """50 positions into a candidate list of `count` entries for point `point` (index in its room) of room `room_id`."""
    if count >= K:
        keys = rng_ref.philox4x32_10(np.uint64(0), np.uint64(0), np.uint64(point), np.uint64((PURPOSE_MCP_NEIGHBOR | rng_ref.PURPOSE_PERMKEY) & 0xFF),
                                     seed, room_id)
        return rng_ref.feistel_permute(np.arange(K), count, [int(k) for k in keys])
    j = np.arange(K, dtype=np.uint64)
    w = np.stack(rng_ref.philox4x32_10(j >> np.uint64(2), np.uint64(0), np.uint64(point), np.uint64(PURPOSE_MCP_NEIGHBOR), seed, room_id), axis=1)
    w = w[np.arange(K), (j & np.uint64(3)).astype(np.int64)].astype(np.uint64)
    return ((w * np.uint64(count)) >> np.uint64(32)).astype(np.int64)


def counter_neighbors(cands, seed, room_id):
    return np.array([c[counter_positions(len(c), seed, room_id, i)] for i, c in enumerate(cands)], dtype=np.int64).reshape(-1, K)


def forward(weights, points, nbr, dtype=np.float64, chunk=2048):
    """dict(h1 [n, 50, 200], h2 [n, 50, 200], pool [n, 200], fc3 [n, 200], fc4 [n, 10], emb [n, 10]) in `dtype`; the inputs are the
    float32 differences points[nbr, :6] - points[i, :6] (:105-106)."""
    w = {k: np.asarray(v, dtype=dtype) for k, v in weights.items()}
    p = np.asarray(points, dtype=np.float32)
    out = {k: [] for k in ('h1', 'h2', 'pool', 'fc3', 'fc4', 'emb')}
    for s in range(0, len(p), chunk):
        idx = np.arange(s, min(len(p), s + chunk))
        x = (p[nbr[idx], :6] - p[idx, None, :6]).astype(dtype)
        h1 = np.maximum(x @ w['mcp_kernel1'][0] + w['mcp_bias1'], 0)
        h2 = np.maximum(h1 @ w['mcp_kernel2'][0] + w['mcp_bias2'], 0)
        pool = h2.max(axis=1)
        cat = np.concatenate([p[idx, 2:6].astype(dtype), pool], axis=1)
        fc3 = np.maximum(cat @ w['mcp_kernel3'] + w['mcp_bias3'], 0)
        fc4 = fc3 @ w['mcp_kernel4'] + w['mcp_bias4']
        emb = fc4 / np.sqrt(np.maximum((fc4 * fc4).sum(axis=1, keepdims=True), 1e-12))
        for k, v in (('h1', h1), ('h2', h2), ('pool', pool), ('fc3', fc3), ('fc4', fc4), ('emb', emb)):
            out[k].append(v)
    return {k: np.concatenate(v) if v else np.zeros((0,)) for k, v in out.items()}


def seq_dot(a, b):
    """Row-wise float64 dot of float32 rows, products exact, summed in order ((p0 + p1) + p2) + ..."""
    pr = np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)
    d = pr[:, 0].copy()
    for c in range(1, pr.shape[1]):
        d = d + pr[:, c]
    return d


def edge_pairs(points, emb, resolution=0.1):
    """(i, k, dot) for every 26-neighbour pair k < i of the voxel graph."""
    nb = baselines_ref.neighbours(points, resolution)
    ii, oo = np.nonzero(nb >= 0)
    kk = nb[ii, oo]
    sel = kk < ii
    ii, kk = ii[sel], kk[sel]
    return ii, kk, seq_dot(np.asarray(emb, np.float32)[kk], np.asarray(emb, np.float32)[ii])


def components(points, emb, threshold=0.9, min_cluster_size=10, resolution=0.1):
    """cluster_label of :136-145: components of the edge graph with more than min_cluster_size points, numbered by smallest index."""
    n = len(points)
    ii, kk, d = edge_pairs(points, emb, resolution)
    e = d > threshold
    root = baselines_ref._roots(n, ii[e], kk[e])
    size = np.bincount(root, minlength=n)
    kept = np.nonzero((size > min_cluster_size) & (np.arange(n) == root))[0]
    ids = np.zeros(n, dtype=np.int64)
    ids[kept] = np.arange(1, len(kept) + 1)
    return ids[root]


def room_metrics(obj_id, cluster_label):
    """:146-170 with mask arithmetic per (instance, cluster) pair, instances in set(obj_id) order: (prc, rcl, iou, cluster_label2)."""
    n_cl = int(cluster_label.max())
    taken = np.zeros(n_cl, dtype=bool)
    relabel = np.zeros(len(cluster_label), dtype=int)
    best, hits = [], 0
    for inst in set(obj_id):
        g = obj_id == inst
        top = 0
        for c in range(1, n_cl + 1):
            if taken[c - 1]:
                continue
            m = cluster_label == c
            score = 1.0 * np.count_nonzero(g & m) / np.count_nonzero(g | m)
            top = max(top, score)
            if score > 0.5:
                taken[c - 1] = True
                hits += 1
                relabel[m] = inst
                break
        best.append(top)
    for c in np.nonzero(~taken)[0] + 1:
        relabel[cluster_label == c] = c + obj_id.max()
    with np.errstate(all='ignore'):
        prc = np.mean(taken)
    return prc, 1.0 * hits / len(set(obj_id)), np.mean(best), relabel


def ply_points(centred, unequalized_idx, emb, cluster_label2):
    """The two clouds :184-193 writes: (embedding-coloured, result-coloured) float32 [M, 6] copies of the centred room."""
    from sklearn.decomposition import PCA
    x = PCA(n_components=3).fit_transform(np.asarray(emb, dtype=np.float64))
    col = (x - x.min(axis=0)) / (x.max(axis=0) - x.min(axis=0)) * 255
    a = np.array(centred, dtype=np.float32)
    a[:, 3:6] = col[unequalized_idx]
    b = np.array(a)
    oc = np.random.RandomState(0).randint(0, 255, (np.max(cluster_label2) + 1, 3))
    b[:, 3:6] = oc[cluster_label2, :][unequalized_idx]
    return a, b


def ply_text(points):
    """What io.savePLY (learn_region_grow_util.py:57-73) writes."""
    head = ("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % len(points))
    return head + ''.join("%f %f %f %d %d %d\n" % (p[0], p[1], p[2], p[3], p[4], p[5]) for p in points)


def nbr_digest(nbrs):
    h = hashlib.sha256()
    for a in nbrs:
        h.update(np.ascontiguousarray(a, dtype=np.int32).tobytes())
    return h.hexdigest()


if __name__ == '__main__':
    sys.exit(__doc__)
