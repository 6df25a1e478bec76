"""Rooms whose regions stop at exactly the size boundaries of the medians (csrc/lrg_median.h and its four callers), host only.

An object is a strip one voxel thick: `count` points fill columns of W voxels (along y), column after column along x; its corner
point comes first in the seed order.  Three points of another object -- the fence -- sit at the far end of the column right after
the strip's last full column.  Under ground-truth masks a region grown from the corner takes every candidate (a step offers at most
2k + 1 of them, 511 at W = 256: below a full set, so no draw decides anything), fills the strip exactly, finds only the fence in its
dilated box and takes one more evaluated step at nc == count, which stops it with 'noexpand': the median IS taken at the full size.
Strips lie 3 empty voxels apart in y, so no dilated box ever reaches another strip.

Channels 0 / 1 are the geometry; channels 6 .. 12 carry the value patterns of test_medians_of_large_regions (smooth; sorted along the
list; two-valued; constant; constant but for a few outliers; negative and clustered near zero; heavy duplicates)."""
import numpy as np

RES = 0.1
CLASSES = [(16, 256), (16, 257), (32, 1024), (32, 1025), (64, 4096), (64, 4097), (128, 16384), (128, 16385)]      # 43 548 points, 500 steps
BIG = [(256, 49152), (256, 49153)]                                                                                # 98 311 points, 516 steps
EVEN = [(256, 49664)]       # 49 667 points, 258 steps: 194 lines of 256, so every size past the square of 194 is even -- 49276, 49470, 49664 above 49152
SIZE_CLASSES = [(1, 256), (257, 1024), (1025, 4096), (4097, 16384), (16385, 49152), (49153, 1 << 30)]
WIDE_SHIFT = 2100           # voxels in y: past the 2048 that packed voxel words hold


def make(strips, wide=False, F=13, room_id=0, seed=7):
    """-> room dict (points [n,F] float32, obj_id, order, room_id) plus 'strips': per strip (first index, W, count).
    wide: the first strip lies WIDE_SHIFT voxels further in y than it would (the room then has no packed voxel words); a room of one
    strip gets a lone point of an object of its own at the origin, last in every order, to be that far from."""
    vox, obj, first = [], [], []
    y0 = WIDE_SHIFT if wide else 0
    for k, (W, count) in enumerate(strips):
        i = np.arange(count)
        first.append(sum(len(v) for v in vox))
        vox.append(np.stack([i // W, y0 + i % W], axis=1))
        obj.append(np.full(count, 2 * k + 1))
        col = count // W                       # the column right after the last full one (a partial last column: that one, at its far end)
        vox.append(np.stack([np.full(3, col), y0 + W - 3 + np.arange(3)], axis=1))
        obj.append(np.full(3, 2 * k + 2))
        y0 = (0 if (wide and k == 0) else y0) + W + 3
    if wide and len(strips) == 1:
        vox.append(np.zeros((1, 2), dtype=vox[0].dtype))
        obj.append(np.full(1, 2 * len(strips) + 1))
    vox = np.concatenate(vox)
    obj = np.concatenate(obj).astype(np.int32)
    n = len(vox)
    rs = np.random.RandomState(seed)
    pts = np.zeros((n, 13), dtype=np.float32)
    pts[:, 0] = vox[:, 0] * 0.1 + 0.03          # one point per 0.1 m voxel
    pts[:, 1] = vox[:, 1] * 0.1 + 0.04
    pts[:, 2] = 0.05
    pts[:, 3] = vox[:, 0] / max(1.0, float(vox[:, 0].max()))
    pts[:, 4] = vox[:, 1] / max(1.0, float(vox[:, 1].max()))
    pts[:, 5] = 0.5
    pts[:, 6] = rs.rand(n)                                           # smooth
    pts[:, 7] = np.sort(rs.randn(n)).astype(np.float32)              # sorted along the list
    pts[:, 8] = (rs.rand(n) < 0.5)                                   # two values
    pts[:, 9] = 0.25                                                 # constant
    pts[:, 10] = np.where(rs.rand(n) < 0.001, rs.randn(n), 1.0)      # constant but for a few outliers
    pts[:, 11] = -np.abs(rs.randn(n)) * 1e-3                         # negative, clustered near zero
    pts[:, 12] = rs.randint(0, 50, n) * 0.5                          # heavy duplicates
    corners = np.asarray(first)
    rest = np.setdiff1d(np.arange(n), corners)
    order = np.concatenate([corners, rest]).astype(np.int32)
    return dict(points=np.ascontiguousarray(pts[:, :F]), obj_id=obj, order=order, room_id=room_id,
                strips=[(f, W, c) for f, (W, c) in zip(first, strips)])


def classes_room(**kw):
    return make(CLASSES, room_id=kw.pop('room_id', 61), **kw)


def cut_room(**kw):
    """The classes room cut to its six smallest strips (regions up to 4097 points)."""
    return make(CLASSES[:6], room_id=kw.pop('room_id', 62), **kw)


def big_room(**kw):
    return make(BIG, room_id=kw.pop('room_id', 63), **kw)


def even_room(**kw):
    """One strip with over ninety even counts above 16 Ki, three of them above 49152: the mean of the two middle keys, where BIG leaves only
    the odd 49153 (a room of its own: a third strip in the big room would pass the packed iteration's 131072 points)."""
    return make(EVEN, room_id=kw.pop('room_id', 64), **kw)


def size_class(nc):
    return next(k for k, (lo, hi) in enumerate(SIZE_CLASSES) if lo <= nc <= hi)


def sampled_bracket(values, nc):
    """lrg_median_block_sampled's pivots restated (csrc/lrg_median.h): a systematic sample of 1024 keys, one per thread, evenly spaced
    over the list; the keys of sample ranks 512 -+ 64 bracket the median.  values: the channel along the region's list.
    -> (keys below the bracket, keys inside it, whether the selection runs inside the bracket: it holds both middle ranks and at most
    8192 keys -- else the full bisection runs)."""
    v = np.asarray(values[:nc])
    samp = np.sort(v[(np.arange(1024, dtype=np.int64) * nc) // 1024])
    plo, phi = samp[512 - 64], samp[512 + 64]
    below = int((v < plo).sum())
    inside = int(((v >= plo) & (v <= phi)).sum())
    k2 = nc >> 1
    k1 = k2 if nc & 1 else k2 - 1
    return below, inside, bool(below <= k1 and k2 < below + inside and inside <= 8192)
