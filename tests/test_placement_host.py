"""Host: the rooms of tests/test_gpu_placement.py are what that file needs them to be (tests/placement_rooms.py).

Conditions on inputs, asserted so that they hold for the seeds chosen: every placement moves whole voxels and keeps them unique, the
oracle labels enough regions for a comparison of regions to mean something, one room has a region above 512 points (one wavefront /
one record of the greedy front) and one above 1024, and the rooms tell the right arithmetic from four plausible wrong ones -- each
planted in a NumPy restatement, never in a kernel."""
import numpy as np
import pytest

import placement_rooms as pr
from oracle import grow_ref


@pytest.fixture(scope='module')
def parts():
    return pr.base_room(*pr.ROOM_A), pr.base_room(*pr.ROOM_B)


@pytest.fixture(scope='module')
def rooms(parts):
    return {name: pr.placed(name, *parts) for name in pr.PLACEMENTS}


@pytest.fixture(scope='module')
def grown(rooms):
    """Every placed room under ground-truth masks and a zero network, once."""
    return {name: pr.oracle(room) for name, room in rooms.items()}


@pytest.mark.parametrize('name', sorted(pr.PLACEMENTS))
def test_place_moves_whole_voxels_and_keeps_them_unique(parts, rooms, name):
    a, b = parts
    room, v = rooms[name], pr.voxels(rooms[name])
    va = pr.voxels(a)
    if name in pr.JOINS:
        axis, extent = 'xyz'.index(name[-1]), {'fits': 0, 'wide': 1}[name[:4]] + pr.PVOX_EXTENT['xyz'.index(name[-1])]
        # the first part stays where it was; the second moved by one whole-voxel step along the join's axis alone
        shift = v[len(va):] - pr.voxels(b)
        assert (shift == shift[0]).all() and (np.delete(shift[0], axis) == 0).all() and shift[0][axis] > 0
        want = np.concatenate([va, pr.voxels(b) + shift[0]])
        assert (v.max(axis=0) - v.min(axis=0))[axis] == extent
        assert room['parts'] == (len(a['points']), len(b['points']))
        np.testing.assert_array_equal(room['order'], np.argsort(room['points'][:, 12], kind='stable'))
        assert not set(room['obj_id'][:len(va)]) & set(room['obj_id'][len(va):])
        np.testing.assert_array_equal(room['points'][:, 3:], np.concatenate([a['points'], b['points']])[:, 3:])
    else:
        want = va + np.asarray(pr.PLACEMENTS[name](a))
        np.testing.assert_array_equal(room['points'][:, 3:], a['points'][:, 3:])
        np.testing.assert_array_equal(room['obj_id'], a['obj_id'])
        np.testing.assert_array_equal(room['order'], a['order'])
    np.testing.assert_array_equal(v, want)
    assert room['points'].dtype == np.float32
    assert len(np.unique(v, axis=0)) == len(v)
    assert pr.has_pvox(room) == (name in pr.KEEP_PVOX)
    if name in pr.NET_POLICY:
        assert np.abs(room['points'][:, 2]).max() < 5.0


def test_placements_are_where_their_names_say(rooms):
    v = {name: pr.voxels(room) for name, room in rooms.items()}
    assert (v['negative'] < 0).all()
    assert (v['straddle'].min(axis=0) < 0).all() and (v['straddle'].max(axis=0) > 0).all()
    assert ((v['straddle'] < 0).sum(axis=0) > 100).all() and ((v['straddle'] > 0).sum(axis=0) > 100).all()
    assert tuple(v['far'].min(axis=0) - pr.voxels(pr.base_room(*pr.ROOM_A)).min(axis=0)) == pr.FAR
    assert v['window'][:, 0].max() == (1 << 20) - 1 and v['window'][:, 1].min() == -(1 << 20)
    assert (pr.hash_key(v['window']) != pr.HASH_EMPTY).all()


@pytest.mark.parametrize('name', sorted(pr.PLACEMENTS))
def test_the_oracle_labels_enough_regions(rooms, grown, name):
    room, res = rooms[name], grown[name]
    labelled = [r for r in res.regions if r['labeled']]
    assert len(labelled) >= 5
    if name in pr.JOINS:
        na = room['parts'][0]
        assert sum(r['seed'] < na for r in labelled) >= 2 and sum(r['seed'] >= na for r in labelled) >= 2


def test_moving_a_room_does_not_change_its_regions(parts, grown):
    """Whole-voxel moves keep the integer side of the loop: same seeds, steps, sizes and stop reasons as at the origin."""
    home = pr.region_tuples(pr.oracle(parts[0]))
    for name in ('negative', 'straddle', 'far', 'window'):
        assert pr.region_tuples(grown[name]) == home, name


def test_regions_above_the_single_wavefront_and_the_set_limits(grown):
    assert max(r['points'] for r in grown['far'].regions) > 512
    big = pr.oracle(pr.base_room(*pr.ROOM_BIG))
    assert max(r['points'] for r in big.regions) > 1024
    assert sum(r['labeled'] for r in big.regions) >= 5
    small = pr.oracle(pr.base_room(*pr.ROOM_SMALL))
    assert sum(r['labeled'] for r in small.regions) >= 5


# ---- planted faults: each changes the oracle's regions or a looked-up index on the room named ----
class UnsignedBox(np.ndarray):
    """Voxel coordinates whose .min / .max along an axis order them as unsigned 32-bit words and return the element found -- the
    box of test_region_grow.py:292-293 as a min / max without the order-preserving flip of the sign bit would give it.  Comparisons,
    arithmetic and numpy.minimum / maximum stay signed."""

    def _pick(self, how, axis):
        plain = np.asarray(self)
        idx = how(plain.astype(np.int64) & 0xFFFFFFFF, axis=axis)
        return np.take_along_axis(plain, np.expand_dims(idx, axis), axis).squeeze(axis)

    def min(self, axis=None, **kw):
        return self._pick(np.argmin, axis)

    def max(self, axis=None, **kw):
        return self._pick(np.argmax, axis)


def test_unsigned_min_max_is_told_apart_on_straddle(rooms, grown, monkeypatch):
    """An unsigned min / max of the members' voxel coordinates, planted in the box computation alone (the oracle's
    point_voxels[mask].min / .max; its neighbour search, voxel keys and everything else stay as they are): a region that crosses
    zero gets its smallest non-negative coordinate as minimum and its largest negative one as maximum.  Invisible at the origin
    and on `far` (no axis changes sign inside a region), visible on `straddle`."""
    right = grow_ref.voxelize
    monkeypatch.setattr(grow_ref, 'voxelize', lambda xyz, resolution: right(xyz, resolution).view(UnsignedBox))
    probe = np.array([[-3, 5, 0], [2, -1, 7]]).view(UnsignedBox)
    assert probe.min(axis=0).tolist() == [2, 5, 0] and probe.max(axis=0).tolist() == [-3, -1, 7]
    assert type(probe[np.array([True, False]), :]) is UnsignedBox          # (what the oracle takes the box of)
    home = pr.base_room(*pr.ROOM_A)
    assert pr.region_tuples(pr.oracle(home)) == pr.region_tuples(grown['far'])          # (same regions as any whole-voxel move of it)
    assert pr.region_tuples(pr.oracle(rooms['far'])) == pr.region_tuples(grown['far'])
    assert pr.region_tuples(pr.oracle(rooms['straddle'])) != pr.region_tuples(grown['straddle'])


def test_round_half_up_is_told_apart_on_the_voxelize_inputs():
    """floor(x / r + 0.5) for rint(x / r): differs on exact halves below an even voxel, which the direct inputs contain at both
    resolutions and on both sides of zero."""
    c = pr.voxelize_coordinates()
    for res in (0.1, 0.3):
        q = c / np.float32(res)
        assert q.dtype == np.float32
        want = grow_ref.voxelize(c, res)
        wrong = np.floor(q + np.float32(0.5)).astype(np.int64)
        d = want != wrong
        assert d.any() and (c[d] > 0).any() and (c[d] < 0).any(), res
    half = np.abs(c / np.float32(0.1) % 1) == 0.5
    assert half.sum() >= 100
    p = pr.voxelize_points(5000, 6, 0)
    assert set(np.unique(c).tolist()) <= set(np.unique(p[:, :3]).tolist())       # (the largest direct case holds every coordinate)


def test_a_hash_key_without_its_offset_is_told_apart_on_negative(parts, rooms):
    """(x << 42 | y << 21 | z) of the coordinates as they are: two's-complement words of negative coordinates run into their
    neighbours' bits, distinct voxels share a key and a lookup returns another point.  At the origin the key is still one-to-one."""
    def plain(v):
        return pr.hash_key(v, offset=0)
    for name, collide in (('negative', True), (None, False)):
        v = pr.voxels(rooms[name] if name else parts[0])
        v = v[(v >= 0).all(axis=1)] if name is None else v
        mask = pr.hash_capacity(len(v)) - 1
        keys, vals = pr.hash_build(v, mask)
        np.testing.assert_array_equal(pr.hash_lookup(keys, vals, mask, pr.hash_key(v)), np.arange(len(v)))
        wkeys, wvals = pr.hash_build(v, mask, key_fn=plain)
        found = pr.hash_lookup(wkeys, wvals, mask, plain(v))
        assert (found != np.arange(len(v))).any() == collide, name


def test_the_packed_word_rule_is_told_apart_on_the_fits_and_wide_pairs(rooms):
    for axis in 'xyz':
        fits, wide = rooms['fits_' + axis], rooms['wide_' + axis]
        assert pr.has_pvox(fits) and not pr.has_pvox(wide)
        assert not pr.has_pvox(fits, over=lambda e, lim: e >= lim)          # '>= 2047' loses the words one voxel early
        assert pr.has_pvox(wide, over=lambda e, lim: e > lim + 1)           # '> 2048' keeps words that no longer fit


def test_the_preview_rule_reads_the_same_extents(rooms):
    """RegionGrower.free_run_applies restates the rule from the host arrays (numpy.rint of the float32 quotient)."""
    for name, room in rooms.items():
        ext = np.ptp(np.rint(room['points'][:, :3] / np.float32(pr.RES)), axis=0)
        assert (not (ext > np.array(pr.PVOX_EXTENT)).any()) == (name in pr.KEEP_PVOX), name
