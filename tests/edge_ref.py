"""NumPy restatement of benchmarks.py --mode edge (:308-353 and :406-436), in two forms.

``literal``  the reference's semantics kept whole (directed edge list in point and offset order with both directions, per-point
             bounds, the criteria, networkx components, the stack search with duplicate pushes and mark-on-pop over stably sorted
             neighbour lists), with ``predict_proba`` replaced by ``mlp_logits`` and ``scipy.special.expit`` (what sklearn calls).
``staged``   what csrc/lrg_edge.hip computes, stage by stage: nb [n, 26], nmin / nmax, F and z per slot [n, 13], p, pmax, the 13-bit
             keep words, cluster labels, stop (the reformulated search), final labels.

The MLP is the ascending-k chain acc = acc + x[k] * W[k][j] from acc = 0, every product and sum rounded, vectorised over rows and
outputs; it does not call BLAS, whose summation order depends on the CPU.
"""
import hashlib
import os

import numpy as np
from scipy.special import expit

from learn_region_grow_amd import preprocess, synthetic
import baselines_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
OFFSETS = baselines_ref.OFFSETS
SLOTS = 13
WEIGHT_KEYS = ('W0', 'b0', 'W1', 'b1', 'W2', 'b2', 'W3', 'b3')


def golden_weights():
    with np.load(os.path.join(GOLDEN, 'edge5_weights.npz')) as z:
        return [z[k] for k in WEIGHT_KEYS]


def raw_rooms():
    """Rooms A and B of tests/golden/edge_ref_cpu.npz, regenerated from their seeds (pinned there by baselines_ref.rooms_digest)."""
    return [synthetic.area5_shaped_room(3000, 3).astype(np.float32), synthetic.generate_room_points(6000, 8).astype(np.float32)]


def equalise(raw, resolution=0.1):
    """benchmarks.py:199-215: the first raw point of every voxel, as a room dict."""
    raw = np.asarray(raw, dtype=np.float32)
    p = preprocess.preprocess_room(raw[:, :6], np.zeros(len(raw), int), np.zeros(len(raw), int), resolution=resolution)
    return dict(points=np.ascontiguousarray(raw[p['equalized_idx'], :6]), equalized_idx=p['equalized_idx'], unequalized_idx=p['unequalized_idx'])


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def mlp_logits(F, weights):
    """[m, 30] float32 -> [m] float64, the value before the logistic function."""
    h = np.asarray(F, dtype=np.float64)
    for l in range(4):
        W, b = weights[2 * l], weights[2 * l + 1]
        acc = np.zeros((len(h), W.shape[1]))
        for k in range(W.shape[0]):
            acc = acc + h[:, k:k + 1] * W[k][None, :]
        acc = acc + b[None, :]
        h = np.maximum(acc, 0.0) if l < 3 else acc
    return h[:, 0]


def edge_rows(a, b, lo_a, lo_b, hi_a, hi_b):
    """The classifier's 30 float32 inputs for the edges between the rows of a and of b ([m, 6] xyzrgb each; lo_* / hi_* are the
    neighbourhood bounds of the same points): mean, smaller and larger of z and rgb; |a - b|; how far either end lies from the other
    end's lower bound, and from its upper bound (the larger of the two distances)."""
    za, zb = a[:, 2:], b[:, 2:]
    blocks = [np.float32(0.5) * (za + zb), np.minimum(za, zb), np.maximum(za, zb), np.abs(a - b),
              np.maximum(np.abs(a - lo_b), np.abs(b - lo_a)), np.maximum(np.abs(a - hi_b), np.abs(b - hi_a))]
    return np.concatenate(blocks, axis=1)


def literal(points, weights, resolution=0.1, min_cluster_size=10, rel=0.99, floor=0.9, probs_fn=None):
    """The semantics of benchmarks.py:325-353 and :406-436 kept whole, nothing reformulated: a directed edge list in (point, offset)
    order with both directions, one probability per directed edge, the criteria, networkx's component order, and the fallback on a
    stack that takes duplicate pushes and marks a node when it is popped, its neighbour lists in edge-list order under a stable
    ascending sort by probability.  Returns dict(labels, n_clusters, E [m, 2], probs [m], pops [the longest search])."""
    import networkx as nx
    from operator import itemgetter
    pts = np.asarray(points, dtype=np.float32)[:, :6]
    n = len(pts)
    nb = baselines_ref.neighbours(pts, resolution)
    src, off = np.nonzero(nb >= 0)                           # row-major: by point, then by offset
    dst = nb[src, off]
    m = len(src)
    label = np.zeros(n, dtype=int)
    if m == 0:
        return dict(labels=label, n_clusters=0, E=np.zeros((0, 2), int), probs=np.zeros(0), pops=0)
    lo, hi = pts.copy(), pts.copy()                          # bounds over the point and every point it shares an edge with
    np.minimum.at(lo, src, pts[dst])
    np.maximum.at(hi, src, pts[dst])
    rows = edge_rows(pts[src], pts[dst], lo[src], lo[dst], hi[src], hi[dst])
    prob = probs_fn(rows) if probs_fn is not None else expit(mlp_logits(rows, weights))
    top = np.zeros(n)                                        # the largest probability met at a point, at least 0
    np.maximum.at(top, src, prob)
    np.maximum.at(top, dst, prob)
    passed = (prob > rel * top[src]) & (prob > rel * top[dst]) & (prob > floor)
    graph = nx.Graph()
    graph.add_edges_from(zip(src[passed].tolist(), dst[passed].tolist()))
    n_clusters = 0
    for members in nx.connected_components(graph):           # in the order the graph first met a member
        if len(members) > min_cluster_size:
            n_clusters += 1
            label[list(members)] = n_clusters
    incident = [[] for _ in range(n)]                        # every directed edge is entered at both of its ends, in list order
    for r in range(m):
        u, v, pr = int(src[r]), int(dst[r]), prob[r]
        incident[u].append((pr, v))
        incident[v].append((pr, u))
    ranked = [[v for _, v in sorted(lst, key=itemgetter(0))] for lst in incident]        # sorted() is stable: ties stay in list order
    longest = 0
    for start in np.flatnonzero(label == 0).tolist():        # the unlabelled points as they stand now; earlier ones get labels meanwhile
        done, pending, pops = set(), [start], 0
        while pending:
            node = pending.pop()
            pops += 1
            if node in done:
                continue
            if label[node] > 0:
                label[start] = label[node]
                break
            done.add(node)
            pending += ranked[node]
        longest = max(longest, pops)
    return dict(labels=label, n_clusters=n_clusters, E=np.stack([src, dst], axis=1), probs=prob, pops=longest)


# ---- the staged form ----

def bounds(points, nb):
    """nmin, nmax [n, 6] float32 over the point and its neighbours."""
    mn, mx = points[:, :6].copy(), points[:, :6].copy()
    for o in range(26):
        k = nb[:, o]
        have = k >= 0
        mn[have] = np.minimum(mn[have], points[k[have], :6])
        mx[have] = np.maximum(mx[have], points[k[have], :6])
    return mn, mx


def slot_logits(points, nb, nmin, nmax, weights):
    """F [n, 13, 30] float32 and z [n, 13] float64, NaN where the neighbour at offset 13 + s is missing."""
    n = len(points)
    F = np.full((n, SLOTS, 30), np.nan, dtype=np.float32)
    z = np.full((n, SLOTS), np.nan)
    ii, ss = np.nonzero(nb[:, 13:] >= 0)
    if len(ii):
        kk = nb[ii, 13 + ss]
        rows = edge_rows(points[ii, :6], points[kk, :6], nmin[ii], nmin[kk], nmax[ii], nmax[kk])
        F[ii, ss] = rows
        z[ii, ss] = mlp_logits(rows, weights)
    return F, z


def edge_probs(p, nb):
    """[n, 26]: the probability of the edge to the neighbour at every offset (0 where there is none)."""
    n = len(nb)
    pe = np.zeros((n, 26))
    for o in range(26):
        have = nb[:, o] >= 0
        if o >= 13:
            pe[have, o] = p[have, o - 13]
        else:
            pe[have, o] = p[nb[have, o], 12 - o]
    return pe


def keep_words(p, nb, rel=0.99, floor=0.9):
    """pmax [n] and the 13-bit keep words [n] uint32 (:346-352)."""
    pe = edge_probs(p, nb)
    pmax = np.max(np.where(nb >= 0, pe, 0.0), axis=1, initial=0.0)
    keep = np.zeros(len(nb), dtype=np.uint32)
    for s in range(SLOTS):
        k = nb[:, 13 + s]
        have = k >= 0
        ps = p[have, s]
        ok = (ps > rel * pmax[have]) & (ps > rel * pmax[k[have]]) & (ps > floor)
        keep[np.nonzero(have)[0][ok]] |= np.uint32(1 << s)
    return pmax, keep


def cluster_labels(keep, nb, min_cluster_size=10):
    """Components of the kept edges with more than min_cluster_size points, numbered by their smallest point (networkx's order on
    E[criteria], which is built in increasing i with both directions: DESIGN.md §3.8)."""
    n = len(nb)
    ii, ss = np.nonzero((keep[:, None] >> np.arange(SLOTS, dtype=np.uint32)[None, :]) & 1)
    root = baselines_ref._roots(n, ii, nb[ii, 13 + ss])
    size = np.bincount(root, minlength=n)
    kept = np.nonzero((size > min_cluster_size) & (np.arange(n) == root))[0]
    ids = np.zeros(n, dtype=np.int64)
    ids[kept] = np.arange(1, len(kept) + 1)
    return ids[root], len(kept)


def live_points(nb, clab):
    """True for the points of voxel-graph components that hold a clustered point."""
    n = len(nb)
    ii, oo = np.nonzero(nb >= 0)
    kk = nb[ii, oo]
    sel = kk < ii
    root = baselines_ref._roots(n, ii[sel], kk[sel])
    has = np.zeros(n, dtype=bool)
    has[root[clab > 0]] = True
    return has[root]


def search_stop(i, nb, pe, clab, cap=None):
    """The reformulated search from i: a recursive DFS that takes the neighbours b of q in descending (p, b > q ? (1, b) : (0, offset)),
    each once, and ends at the first x != i that is clustered or (unlabelled and x < i).  Returns (x, visited count); -2 past cap."""
    visited = {i}
    result = []

    def visit(q):
        order = sorted((o for o in range(26) if nb[q, o] >= 0),
                       key=lambda o: (pe[q, o], (1, int(nb[q, o])) if nb[q, o] > q else (0, o)), reverse=True)
        for o in order:
            x = int(nb[q, o])
            if x in visited:
                continue
            if clab[x] > 0 or x < i:
                result.append(x)
                return True
            if cap is not None and len(visited) >= cap:
                result.append(-2)
                return True
            visited.add(x)
            if visit(x):
                return True
        return False
    import sys
    lim = sys.getrecursionlimit()
    sys.setrecursionlimit(max(lim, 20000))
    try:
        visit(i)
    finally:
        sys.setrecursionlimit(lim)
    return (result[0] if result else -1), len(visited)


def stops(nb, p, clab, cap=None):
    """stop [n] int32 (-1: no search, -2: past cap) and the largest visited set."""
    pe = edge_probs(p, nb)
    live = live_points(nb, clab)
    stop = np.full(len(nb), -1, dtype=np.int32)
    largest = 0
    for i in np.nonzero((clab == 0) & live)[0]:
        stop[i], v = search_stop(int(i), nb, pe, clab, cap)
        largest = max(largest, v)
    return stop, live, largest


def resolve(clab, stop):
    label = np.array(clab, dtype=np.int64)
    for i in np.nonzero(stop >= 0)[0]:
        label[i] = label[stop[i]]
    return label


def staged(points, weights, resolution=0.1, min_cluster_size=10, rel=0.99, floor=0.9, p=None, cap=None):
    """Every stage of one room.  p given: the stages after the logistic function on those probabilities."""
    points = np.asarray(points, dtype=np.float32)
    nb = baselines_ref.neighbours(points, resolution)
    nmin, nmax = bounds(points, nb)
    out = dict(nb=nb, nmin=nmin, nmax=nmax)
    if p is None:
        out['F'], out['z'] = slot_logits(points, nb, nmin, nmax, weights)
        p = expit(out['z'])
    out['p'] = p
    out['pmax'], out['keep'] = keep_words(p, nb, rel, floor)
    out['cluster_labels'], out['n_clusters'] = cluster_labels(out['keep'], nb, min_cluster_size)
    out['stop'], out['live'], out['largest_visited'] = stops(nb, p, out['cluster_labels'], cap)
    out['labels'] = resolve(out['cluster_labels'], out['stop'])
    return out
