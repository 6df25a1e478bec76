"""NumPy twin of the FPFH mode (learn_region_grow_amd.baselines.fpfh and segment(..., 'fpfh')).

The definition, stage by stage, vectorised over the pairs of a room:
  inputs      points[:, :3] and float32(normals) through the PCD round trip by the string route (``roundtrip_str``)
  window      the point of every voxel within +-2 of a point's own (``window``; voxels from the points BEFORE the round trip)
  ball        d2 = (dx dx + dy dy) + dz dz <= r2 in float32 (``twin``: I, J, d2, k)
  pairs       PCL's computePairFeatures and the three bins, in float32 and in float64 from the same float32 inputs (``pair_features``)
  near        per pair, in float64: a scaled feature within DELTA of an interior bin boundary, ||a1| - |a2|| < DELTA (an exact tie of
              bitwise-equal normals excepted), hypot of atan2's arguments < 1e-2, |v| < 1e-6, |d2 - r2| < 1e-6 r2 (this last one for
              every candidate of the window, in the ball or not).  A point with a near pair is *excused*: float32 arithmetic that
              differs from this twin's in its last bits (atan2f, the order of a sum) may bin such a pair differently.
  descriptor  ``fpfh_from_counts``: SPFH = count * (100 / (k - 1)) in float32, the 1 / d2 weighted sum over the neighbours in window order (the
              point's own SPFH is not added), each block of 11 scaled to sum 100
  edge        ``unit`` and ``edge``: float64, sums in order; clustering with baselines_ref's neighbour table and union-find
"""
import itertools
import sys

import numpy as np

import baselines_ref as R

WINDOW = list(itertools.product(range(-2, 3), repeat=3))          # 125 offsets, the point's own voxel at index 62
DELTA = 1e-4                                                     # ten times the float32 error of a scaled feature (a few ulps of O(1), times 11)
BINS = 33


def roundtrip_str(a):
    """float32(float('%f' % v)) for every element: savePCD's print, PCL's parse."""
    a = np.asarray(a, dtype=np.float32)
    return np.array([float('%f' % v) for v in a.ravel().tolist()], dtype=np.float64).astype(np.float32).reshape(a.shape)


def inputs(room):
    """(P, n): the float32 coordinates and normals the descriptor is computed from."""
    return roundtrip_str(np.asarray(room['points'])[:, :3]), roundtrip_str(np.asarray(room['normals'], dtype=np.float64).astype(np.float32))


def window(points, resolution):
    """[N, 125] index of the point in each voxel of the +-2 window (WINDOW order; column 62 is the point itself), -1 where empty."""
    v = np.round(np.asarray(points, np.float32)[:, :3] / np.float32(resolution)).astype(np.int64)
    key = lambda w: ((w[:, 0] + R.VOX_OFF) << 42) | ((w[:, 1] + R.VOX_OFF) << 21) | (w[:, 2] + R.VOX_OFF)
    k = key(v)
    order = np.argsort(k, kind='stable')
    sk = k[order]
    if len(sk) > 1 and (np.diff(sk) == 0).any():
        raise ValueError('two points share a voxel: the room is not equalised')
    nb = np.full((len(v), len(WINDOW)), -1, dtype=np.int64)
    for o, off in enumerate(WINDOW):
        q = key(v + np.array(off))
        pos = np.minimum(np.searchsorted(sk, q), max(len(sk) - 1, 0))
        hit = sk[pos] == q if len(sk) else np.zeros(0, bool)
        nb[hit, o] = order[pos[hit]]
    return nb


def dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def cross3(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def pair_features(P, n, I, J, dtype):
    """computePairFeatures for p1 = P[I], p2 = P[J] (I != J) in `dtype`.  Returns dict(ok [m] bool: not skipped; bins [m, 3] int;
    scaled [m, 3]: 11 * the normalised features; a1, a2; atan_args [m, 2]; vnorm)."""
    T = dtype
    P, n = P.astype(T), n.astype(T)
    with np.errstate(all='ignore'):
        d = P[J] - P[I]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        f4 = np.sqrt(d2)
        ok = f4 != 0
        n1, n2 = n[I], n[J]
        a1, a2 = dot3(n1, d) / f4, dot3(n2, d) / f4
        swap = np.abs(a1) < np.abs(a2)                        # strict: a tie does not swap
        s = swap[:, None]
        n1, n2, d = np.where(s, n2, n1), np.where(s, n1, n2), np.where(s, -d, d)
        f3 = np.where(swap, -a2, a1)
        v = cross3(d, n1)
        vn = np.sqrt(dot3(v, v))
        ok &= vn != 0
        v = v / vn[:, None]
        w = cross3(n1, v)
        f2 = dot3(v, n2)
        y, x = dot3(w, n2), dot3(n1, n2)
        f1 = np.arctan2(y, x)
        pi = T(np.pi)
        scaled = np.stack([T(11) * ((f1 + pi) / (T(2) * pi)), T(11) * ((f2 + T(1)) / T(2)), T(11) * ((f3 + T(1)) / T(2))], axis=1)
        bins = np.clip(np.floor(np.where(np.isnan(scaled), T(0), scaled)), 0, 10).astype(np.int64)
    return dict(ok=ok, bins=bins, scaled=scaled, a1=a1, a2=a2, atan_args=np.stack([y, x], axis=1), vnorm=vn)


def histogram(N, I, bins, ok):
    """counts [N, 33] int32: c[b1], c[11 + b2], c[22 + b3] incremented for every pair that was not skipped."""
    c = np.zeros(N * BINS, dtype=np.int64)
    for g in range(3):
        c += np.bincount(I[ok] * BINS + 11 * g + bins[ok, g], minlength=N * BINS)
    return c.reshape(N, BINS).astype(np.int32)


def twin(room, resolution=0.1, radius=None):
    """Everything up to the counts.  Returns dict(P, n, N, I, J, d2 (the ball's pairs j != i in window order, d2 float32), k [N],
    counts32, counts64 [N, 33], ok32 / ok64 per pair, pairs [N]: non-skipped pairs per point (float64), near [m] per pair,
    near_pairs [N]: near candidates per point (those outside the ball included), excused [N], window: the [N, 125] table)."""
    radius = 2 * resolution if radius is None else radius
    P, n = inputs(room)
    N = len(P)
    nbw = window(room['points'], resolution)
    r2 = np.float32(radius) * np.float32(radius)
    I, S = np.nonzero(nbw >= 0)                               # row-major: by point, then in window order
    J = nbw[I, S]
    d = P[J] - P[I]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    inb = d2 <= r2
    k = np.bincount(I[inb], minlength=N).astype(np.int32)
    d64 = P[J].astype(np.float64) - P[I].astype(np.float64)
    d2_64 = (d64[:, 0] * d64[:, 0] + d64[:, 1] * d64[:, 1]) + d64[:, 2] * d64[:, 2]
    other = J != I
    near_radius = other & (np.abs(d2_64 - np.float64(r2)) < 1e-6 * np.float64(r2))
    pair = inb & other
    near_cand = near_radius.copy()
    I, J, d2 = I[pair], J[pair], d2[pair]
    f32, f64 = pair_features(P, n, I, J, np.float32), pair_features(P, n, I, J, np.float64)
    sc = f64['scaled']
    rb = np.rint(sc)
    with np.errstate(invalid='ignore'):
        near = ((np.abs(sc - rb) < DELTA) & (rb >= 1) & (rb <= 10)).any(axis=1)
        same_normal = (n[I].view(np.uint32) == n[J].view(np.uint32)).all(axis=1)
        near |= (np.abs(np.abs(f64['a1']) - np.abs(f64['a2'])) < DELTA) & ~(same_normal & (f64['a1'] == f64['a2']))
        near |= np.hypot(f64['atan_args'][:, 0], f64['atan_args'][:, 1]) < 1e-2
        near |= ~(f64['vnorm'] >= 1e-6)
    near_cand[np.nonzero(pair)[0][near]] = True
    near_pairs = np.bincount(np.nonzero(nbw >= 0)[0][near_cand], minlength=N)
    return dict(P=P, n=n, N=N, I=I, J=J, d2=d2, k=k, ok32=f32['ok'], ok64=f64['ok'], bins32=f32['bins'], bins64=f64['bins'],
                counts32=histogram(N, I, f32['bins'], f32['ok']), counts64=histogram(N, I, f64['bins'], f64['ok']),
                pairs=np.bincount(I[f64['ok']], minlength=N), near=near | near_radius[pair], near_pairs=near_pairs,
                excused=near_pairs > 0, window=nbw)


def fpfh_from_counts(counts, k, I, J, d2, dtype=np.float64):
    """The descriptor [N, 33] from counts [N, 33], k [N] and the ball's pairs (I, J, d2 float32; j != i, sorted by I, a point's pairs in
    window order).  The SPFH is float32, as defined; weights, the sum (pair by pair in that order) and the scaling are in `dtype`,
    which is also the dtype of the result."""
    T = dtype
    N = len(k)
    with np.errstate(all='ignore'):
        scale = np.where(k > 1, np.float32(100) / (k - 1).astype(np.float32), np.float32(0)).astype(np.float32)
        spfh = (counts.astype(np.float32) * scale[:, None]).astype(T)
        wgt = T(1) / d2.astype(T)
        acc = np.zeros((N, BINS), dtype=T)
        first = np.searchsorted(I, np.arange(N))
        pos = np.arange(len(I)) - first[I]
        for q in range(int(pos.max()) + 1 if len(I) else 0):
            sel = pos == q
            acc[I[sel]] += spfh[J[sel]] * wgt[sel][:, None]
        out = acc.copy()
        for g in range(3):
            s = np.zeros(N, dtype=T)
            for b in range(11):
                s = s + acc[:, 11 * g + b]
            nz = s != 0
            f = T(100) / s[nz]
            out[nz, 11 * g:11 * g + 11] = acc[nz, 11 * g:11 * g + 11] * f[:, None]
    return out


def describe(room, resolution=0.1, radius=None):
    """The twin's own descriptor as float32: float32 pair features, float64 sums."""
    t = twin(room, resolution, radius)
    return fpfh_from_counts(t['counts32'], t['k'], t['I'], t['J'], t['d2'], np.float64).astype(np.float32)


def unit(hist):
    """u = double(h) / sqrt(sum of double(h[d])^2 over d = 0 .. 32 in that order); NaN rows for zero histograms."""
    h = np.asarray(hist, dtype=np.float32).astype(np.float64)
    s = np.zeros(len(h))
    for d in range(BINS):
        s = s + h[:, d] * h[:, d]
    with np.errstate(invalid='ignore', divide='ignore'):
        return h / np.sqrt(s)[:, None]


def edge(u, i, k, t):
    a, b = u[k], u[i]
    dot = a[:, 0] * b[:, 0]
    for d in range(1, BINS):
        dot = dot + a[:, d] * b[:, d]
    with np.errstate(invalid='ignore'):
        return dot > t


def segment(points, hist, t, resolution=0.1, min_cluster_size=10):
    """cluster labels of one room from its histograms: the 26-neighbour voxel graph, the float64 edge, components of more than
    min_cluster_size points numbered by their smallest point index (networkx's order)."""
    n = len(points)
    nb = R.neighbours(np.asarray(points, np.float32), resolution)
    ii, oo = np.nonzero(nb >= 0)
    kk = nb[ii, oo]
    sel = kk < ii
    ii, kk = ii[sel], kk[sel]
    e = edge(unit(hist), ii, kk, t) if n else np.zeros(0, bool)
    root = R._roots(n, ii[e], kk[e])
    size = np.bincount(root, minlength=n)
    kept = np.nonzero((size > min_cluster_size) & (np.arange(n) == root))[0]
    ids = np.zeros(n, dtype=np.int64)
    ids[kept] = np.arange(1, len(kept) + 1)
    return ids[root] if n else ids


def make_room(xyz, normals=None):
    """A hand-built equalised room: points [N, 6] float32 (zero colour) and float64 normals (default (0, 0, 1))."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    normals = np.tile([0.0, 0.0, 1.0], (n, 1)) if normals is None else np.asarray(normals, np.float64)
    return dict(points=np.hstack([xyz, np.zeros((n, 3), np.float32)]).astype(np.float32), normals=normals)


def flat_patch(side=12, spacing=0.1):
    """side x side grid in the plane z = 0, normals (0, 0, 1): every pair has f1 = f2 = f3 = 0, i.e. bins 5, 16 and 27."""
    g = np.arange(side) * spacing
    x, y = np.meshgrid(g, g, indexing='ij')
    return make_room(np.stack([x.ravel(), y.ravel(), np.zeros(side * side)], axis=1))


if __name__ == '__main__':
    sys.exit(__doc__)
