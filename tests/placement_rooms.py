"""Rooms away from the origin: host helpers of tests/test_placement_host.py and tests/test_gpu_placement.py.

The generators of learn_region_grow_amd.synthetic build every room with one corner at (0, 0, 0), so its voxel coordinates
(test_region_grow.py:175) lie between -1 and ~150.  Real rooms keep their building coordinates.  `place` moves an equalised room by a
whole number of voxels, `join` makes one room of two, and PLACEMENTS names where the tests put them: below zero on every axis, across
zero, far out, at the corners of the 21-bit window of the voxel hash keys, and at joint extents one below and one past what the packed
voxel words hold (2048 x 2048 x 1024 voxels)."""
import numpy as np

from learn_region_grow_amd import preprocess, synthetic
from oracle import grow_ref, rng_ref

RES = 0.1
VOX_OFF = 1 << 20                       # the voxel hash keys hold coordinates of -2^20 .. 2^20 - 1
PVOX_EXTENT = (2047, 2047, 1023)        # the largest max - min per axis that packed voxel words hold
FAR = (1637, -2041, 402)


def base_room(seed, n_eq, furniture, room_id=0):
    """An equalised Area-5-shaped room at the origin (host preprocessing)."""
    raw = synthetic.area5_shaped_room(n_eq, seed, n_furniture=furniture).astype(np.float32)
    p = preprocess.preprocess_room(raw[:, :6], raw[:, 6].astype(int), raw[:, 7].astype(int))
    return dict(points=p['points'], obj_id=p['obj_id'], order=p['order'], room_id=room_id)


def voxels(room):
    return grow_ref.voxelize(room['points'][:, :3], RES)


def place(room, K):
    """The room moved by K whole voxels: every point keeps 0.8 of its offset from its voxel's centre, so that the points that shared no
    voxel before share none after, whatever float32 spacing the new coordinates have.  Moves xyz only."""
    K = np.asarray(K, dtype=np.int64)
    x = np.asarray(room['points'][:, :3], dtype=np.float32)
    v = grow_ref.voxelize(x, RES)
    moved = ((v + K) * 0.1).astype(np.float32) + np.float32(0.8) * (x - (v * 0.1).astype(np.float32))
    assert moved.dtype == np.float32
    pts = room['points'].copy()
    pts[:, :3] = moved
    out = dict(room, points=pts)
    got = voxels(out)
    assert (got == v + K).all(), 'place(%s): %d points left their voxel' % (K.tolist(), int((got != v + K).any(axis=1).sum()))
    return out


def join(a, b):
    """One room of two: b's instances are numbered after a's, seeds are visited by curvature (test_region_grow.py:183)."""
    pts = np.concatenate([a['points'], b['points']])
    obj = np.concatenate([np.asarray(a['obj_id']), np.asarray(b['obj_id']) + int(np.max(a['obj_id'])) + 1]).astype(np.int32)
    return dict(points=pts, obj_id=obj, order=np.argsort(pts[:, 12], kind='stable'), room_id=a['room_id'], parts=(len(a['points']), len(b['points'])))


def _negative(room):
    v = voxels(room)
    return (-int(v[:, 0].max()) - 373, -int(v[:, 1].max()) - 129, -int(v[:, 2].max()) - 2)      # (z stays within 5 m of zero)


def _straddle(room):
    v = voxels(room)
    return tuple(int(-((lo + hi) // 2)) for lo, hi in zip(v.min(axis=0), v.max(axis=0)))


def _window(room):
    v = voxels(room)
    return (VOX_OFF - 1 - int(v[:, 0].max()), -VOX_OFF - int(v[:, 1].min()), 0)


def _spread(axis, extent):
    """A join of two rooms whose voxel box is `extent` = max - min along `axis`."""
    def make(a, b):
        va, vb = voxels(a), voxels(b)
        K = [0, 0, 0]
        K[axis] = int(va[:, axis].min()) + extent - int(vb[:, axis].max())
        return join(a, place(b, K))
    return make


# name -> (one room: room -> K) or (two rooms: (a, b) -> room)
PLACEMENTS = {
    'negative': _negative, 'straddle': _straddle, 'far': lambda room: FAR, 'window': _window,
    'fits_x': _spread(0, 2047), 'fits_y': _spread(1, 2047), 'fits_z': _spread(2, 1023),
    'wide_x': _spread(0, 2048), 'wide_y': _spread(1, 2048), 'wide_z': _spread(2, 1024),
}
JOINS = ('fits_x', 'fits_y', 'fits_z', 'wide_x', 'wide_y', 'wide_z')
KEEP_PVOX = ('negative', 'straddle', 'far', 'window', 'fits_x', 'fits_y', 'fits_z')
WIDE = ('wide_x', 'wide_y', 'wide_z')
# z is not centred before the network (test_region_grow.py:243-247): the Bernoulli policy only where z stays within 5 m of zero
NET_POLICY = ('negative', 'straddle', 'window', 'fits_x', 'fits_y', 'wide_x', 'wide_y')

# the rooms: (seed, equalised points asked for, pieces of furniture); ROOM_B is the second part of the joins
ROOM_A, ROOM_B = (304, 3000, 4), (302, 1500, 3)      # ROOM_A has a region above 512 points under ground-truth masks
ROOM_SMALL = (301, 1500, 4)
ROOM_BIG = (303, 6000, 4)               # under ground-truth masks: regions above 512 and above 1024 points


def placed(name, a=None, b=None, room_id=0):
    """The room of placement `name` (built from ROOM_A, and ROOM_B for the joins, unless given)."""
    a = base_room(*ROOM_A) if a is None else a
    if name in JOINS:
        room = PLACEMENTS[name](a, base_room(*ROOM_B) if b is None else b)
    else:
        room = place(a, PLACEMENTS[name](a))
    return dict(room, room_id=room_id)


def has_pvox(room, over=lambda extent, limit: extent > limit):
    """The rule of RegionGrower.load_rooms: packed voxel words unless an extent is over its limit."""
    v = voxels(room)
    return not any(over(int(e), lim) for e, lim in zip(v.max(axis=0) - v.min(axis=0), PVOX_EXTENT))


def zero_net(xi, xn):
    return np.zeros((1, xn.shape[1], 2), np.float32), np.zeros((1, xi.shape[1], 2), np.float32)


def oracle(room, policy='gt', seed=0, net_fn=zero_net, **kw):
    return grow_ref.grow_room(room['points'], room['obj_id'], room['order'], None, rng_ref.CounterStream(seed, room['room_id']),
                              net_fn=net_fn, policy=policy, **kw)


def region_tuples(res):
    return [(r['seed'], r['steps'], r['points'], r['reason'], r['labeled']) for r in res.regions]


# ---- the inputs of the direct lrg_voxelize test ----
def voxelize_coordinates():
    """float32 coordinates at which rint(x / resolution) can go wrong: k / 4 and k / 20 (exact halves both ways at 0.1), signed zeros,
    denormal-range values, the float32 neighbours of voxel boundaries, values near +-1.04e5 (the window of the hash keys at 0.1 m)."""
    k = np.arange(-400, 401)
    c = [k / 4.0, k / 20.0, [0.0, -0.0, 1e-30, -1e-30]]
    rs = np.random.RandomState(5)
    b = ((rs.randint(-3000, 3000, 200) + 0.5) * 0.1).astype(np.float32)          # 200 voxel boundaries at 0.1
    c += [b, np.nextafter(b, np.float32(np.inf)), np.nextafter(b, np.float32(-np.inf))]
    b3 = ((rs.randint(-1000, 1000, 200) + 0.5) * 0.3).astype(np.float32)         # ... and at 0.3
    c += [b3, np.nextafter(b3, np.float32(np.inf)), np.nextafter(b3, np.float32(-np.inf))]
    far = np.float32(1.04e5) + rs.uniform(-50, 50, 300).astype(np.float32)
    c += [far, -far, [104857.5, -104857.6, 104857.45, -104857.55]]
    return np.concatenate([np.asarray(x, dtype=np.float32) for x in c])


def voxelize_points(n, F, seed):
    """n rows of F columns whose first three are drawn from voxelize_coordinates() (every coordinate is used when n allows)."""
    c = voxelize_coordinates()
    rs = np.random.RandomState(seed)
    p = rs.rand(n, F).astype(np.float32)
    flat = np.concatenate([c, c[rs.randint(0, len(c), max(0, 3 * n - len(c)))]])[:3 * n]
    p[:, :3] = rs.permutation(flat).reshape(n, 3)
    return p


# ---- NumPy restatements of the voxel tables (csrc/lrg_common.h, csrc/lrg_grow.hip) ----
HASH_EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def hash_key(v, offset=VOX_OFF):
    """lrg_pack_voxel: 21 bits per coordinate after adding 2^20; HASH_EMPTY outside the window."""
    v = np.asarray(v, dtype=np.int64)
    u = (v + offset).astype(np.uint32).astype(np.uint64)          # (unsigned)(x + LRG_VOX_OFF)
    out = (u[..., 0] << np.uint64(42)) | (u[..., 1] << np.uint64(21)) | u[..., 2]
    if offset:
        out = np.where(((u[..., 0] | u[..., 1] | u[..., 2]) >> np.uint64(21)) != 0, HASH_EMPTY, out)
    return out


def fmix64(k):
    k = np.asarray(k, dtype=np.uint64).copy()
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xff51afd7ed558ccd)
    k ^= k >> np.uint64(33)
    k *= np.uint64(0xc4ceb9fe1a85ec53)
    k ^= k >> np.uint64(33)
    return k


def hash_lookup(keys, vals, mask, query):
    """lrg_hash_lookup for an array of keys: linear probing from fmix64(key) & mask; -1 = absent."""
    query = np.asarray(query, dtype=np.uint64)
    h = (fmix64(query) & np.uint64(0xFFFFFFFF)).astype(np.int64) & mask
    out = np.full(query.shape, -1, dtype=np.int64)
    live = query != HASH_EMPTY
    for _ in range(mask + 1):
        if not live.any():
            break
        k = keys[h]
        hit = live & (k == query)
        out[hit] = vals[h[hit]]
        live &= ~hit & (k != HASH_EMPTY)
        h = (h + 1) & mask
    return out


def hash_build(v, mask, key_fn=hash_key):
    """A table as lrg_voxel_hash_build leaves it, but for the slots' order among colliding keys (inserted in index order here)."""
    keys = np.full(mask + 1, HASH_EMPTY, dtype=np.uint64)
    vals = np.zeros(mask + 1, dtype=np.int32)
    k = key_fn(v)
    h = (fmix64(k) & np.uint64(0xFFFFFFFF)).astype(np.int64) & mask
    for i in range(len(k)):
        j = int(h[i])
        while keys[j] != HASH_EMPTY and keys[j] != k[i]:
            j = (j + 1) & mask
        if keys[j] == HASH_EMPTY:
            keys[j], vals[j] = k[i], i
    return keys, vals


def hash_capacity(n):
    """The table size RegionGrower.load_rooms gives a room of n points."""
    return max(16, 1 << int(np.ceil(np.log2(2 * n + 1))))
