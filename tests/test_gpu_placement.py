"""GPU: growing away from the origin, and the general one-launch front (lrg_front_kernel<7>).

The generators build every room with a corner at (0, 0, 0); here rooms are moved by whole voxels (tests/placement_rooms.py) below
zero, across zero, far out, to the corners of the hash keys' window and to joint extents of 2047 / 2048 (x, y) and 1023 / 1024 (z)
voxels -- one below and one past what the packed voxel words hold.  Three parts:

  1. the voxel kernels alone through the C-ABI (lrg_voxelize, lrg_voxel_pack, lrg_voxel_grid_build, lrg_voxel_hash_build) against
     NumPy, exactly;
  2. the grow loop at every placement, in every formulation, against the oracle driven by the same GPU network: regions (seed,
     steps, points, stop reason, labelled), labels before and after fill-in, all exactly;
  3. the doors into lrg_front_kernel<7> -- rooms without packed voxel words (wide_*), restarts with group_size = 1, sets above 512.

The (x - c) + c round trip of test_region_grow.py:271-276 is exact away from the origin, so translation exercises the integer and
index machinery; moved voxels stay with test_moved_voxels_take_the_general_form."""
import ctypes

import numpy as np
import pytest

import placement_rooms as pr
from conftest import seed_without_near_tie
from learn_region_grow_amd import synthetic
from oracle import grow_ref
from test_gpu_grow import WEIGHT_KW, SAME_LOGITS_MARGIN, gpu_net_fn, same_regions

pytestmark = pytest.mark.gpu


def _net(cuda_device, ni, nn):
    from learn_region_grow_amd.lrgnet import LrgNetHIP
    return LrgNetHIP(1, 1, ni, nn, 13, 0, device=cuda_device).load_weights(synthetic.make_synthetic_weights(**WEIGHT_KW))


@pytest.fixture(scope='module')
def net(cuda_device):
    return _net(cuda_device, 512, 512)


# =====================================================================================================
# 1. the voxel kernels alone
# =====================================================================================================
def _dev(a, cuda_device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda_device)


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize('n', [1, 255, 256, 257, 5000])
@pytest.mark.parametrize('res', [0.1, 0.3])
@pytest.mark.parametrize('F', [6, 13])
def test_voxelize(hip_lib, cuda_device, F, res, n):
    """rint(x / resolution) in float32, half to even (test_region_grow.py:175), on exact halves both ways, signed zeros, the float32
    neighbours of voxel boundaries and coordinates near +-1.04e5 m; the words behind the last point stay untouched."""
    import torch
    p = pr.voxelize_points(n, F, seed=n + F)
    d_p = _dev(p, cuda_device)
    d_v = torch.full((n * 3 + 5,), -77, dtype=torch.int32, device=cuda_device)
    assert hip_lib.lrg_voxelize(_vp(d_p), n, F, ctypes.c_float(res), _vp(d_v), _stream()) == 0
    got = d_v.cpu().numpy()
    np.testing.assert_array_equal(got[:3 * n].reshape(n, 3), grow_ref.voxelize(p[:, :3], res))
    assert (got[3 * n:] == -77).all()


def _pack_words(v, origin):
    r = np.asarray(v, np.int64) - np.asarray(origin, np.int64)
    return (r[:, 0] | (r[:, 1] << 11) | (r[:, 2] << 22)).astype(np.uint32)


def test_voxel_pack(hip_lib, cuda_device):
    """Words are x | y << 11 | z << 22 relative to the origin; the flag stays 0 at extents of 2047 / 2047 / 1023 and is raised by
    2048 on x alone, 2048 on y alone, 1024 on z alone and by a voxel below the origin on each axis."""
    import torch
    rs = np.random.RandomState(3)
    origin = np.array([-1500, -1500, -600])
    n = 700
    rel = np.stack([rs.randint(0, 2048, n), rs.randint(0, 2048, n), rs.randint(0, 1024, n)], axis=1)
    rel[:4] = [[0, 0, 0], [2047, 0, 0], [0, 2047, 0], [0, 0, 1023]]
    rel[4] = [2047, 2047, 1023]
    flag = torch.zeros(1, dtype=torch.int32, device=cuda_device)

    def run(rel):
        v = (rel + origin).astype(np.int32)
        d_v = _dev(v, cuda_device)
        d_w = torch.full((len(v) + 3,), 0x5A5A5A5A, dtype=torch.int32, device=cuda_device)
        flag.zero_()
        assert hip_lib.lrg_voxel_pack(_vp(d_v), len(v), int(origin[0]), int(origin[1]), int(origin[2]), _vp(d_w), _vp(flag), _stream()) == 0
        w = d_w.cpu().numpy().view(np.uint32)
        assert (w[len(v):] == 0x5A5A5A5A).all()
        return v, w[:len(v)], int(flag.item())

    v, w, f = run(rel)
    assert f == 0
    np.testing.assert_array_equal(w, _pack_words(v, origin))
    for axis, beyond in ((0, 2048), (1, 2048), (2, 1024)):
        for bad in (beyond, -1):
            r2 = rel.copy()
            r2[333] = 0
            r2[333, axis] = bad
            v, w, f = run(r2)
            assert f == 1, (axis, bad)
            ok = np.arange(n) != 333
            np.testing.assert_array_equal(w[ok], _pack_words(v, origin)[ok])
    v, w, f = run(rel)            # (the flag is the caller's to reset: a clean call after the raised ones)
    assert f == 0


@pytest.mark.parametrize('origin,dims,n', [((-385, -141, -35), (37, 1, 29), 300), ((-6, -6, -16), (13, 13, 34), 1888), ((5, -1048576, 0), (1, 1, 1), 1),
                                           ((1048563, -3, -2), (5, 6, 7), 210), ((-2, -2, -2), (1, 300, 1), 257)])
def test_voxel_grid_build(hip_lib, cuda_device, origin, dims, n):
    """The dense grid of a room's box: every occupied cell holds its point, every other cell -1.  RegionGrower hands the call an
    uninitialised buffer (the call clears it), so the buffer starts with junk here and ALL cells are checked; the words behind the
    grid keep the junk.  Negative origins, one-voxel-thick boxes, point counts that are no multiple of 256."""
    import torch
    rs = np.random.RandomState(n)
    gx, gy, gz = dims
    cells = gx * gy * gz
    pick = rs.permutation(cells)[:n]
    rel = np.stack([pick % gx, (pick // gx) % gy, pick // (gx * gy)], axis=1)
    v = (rel + np.asarray(origin)).astype(np.int32)
    d_v = _dev(v, cuda_device)
    d_g = torch.full((cells + 7,), 123456, dtype=torch.int32, device=cuda_device)
    assert hip_lib.lrg_voxel_grid_build(_vp(d_v), n, *[int(x) for x in origin], gx, gy, gz, _vp(d_g), _stream()) == 0
    got = d_g.cpu().numpy()
    want = np.full(cells, -1, np.int32)
    want[pick] = np.arange(n)
    np.testing.assert_array_equal(got[:cells], want)
    assert (got[cells:] == 123456).all()


def _hash_build(hip_lib, cuda_device, v, mask):
    import torch
    d_v = _dev(np.asarray(v, np.int32), cuda_device)
    keys = torch.full((mask + 1 + 4,), 0x1234, dtype=torch.int64, device=cuda_device)
    vals = torch.full((mask + 1 + 4,), -9, dtype=torch.int32, device=cuda_device)
    flag = torch.zeros(1, dtype=torch.int32, device=cuda_device)
    rc = hip_lib.lrg_voxel_hash_build(_vp(d_v), len(v), _vp(keys), _vp(vals), mask, _vp(flag), _stream())
    k, x = keys.cpu().numpy(), vals.cpu().numpy()
    assert (k[mask + 1:] == 0x1234).all() and (x[mask + 1:] == -9).all()
    return rc, k[:mask + 1].view(np.uint64), x[:mask + 1], int(flag.item())


def _check_table(keys, vals, mask, v, present, rs):
    """Lookups (a NumPy restatement of lrg_fmix64 + linear probing) of every point's voxel, its 26 neighbours and 1000 absent
    voxels: the index of the point that lives there, -1 where none does.  present: the points the table must hold."""
    v = np.asarray(v, np.int64)
    truth = {tuple(x): i for i, x in enumerate(v.tolist()) if present[i]}
    assert ((keys != pr.HASH_EMPTY).sum()) == len(truth)
    off = np.stack(np.meshgrid([-1, 0, 1], [-1, 0, 1], [-1, 0, 1], indexing='ij'), -1).reshape(27, 3)
    q = (v[:, None, :] + off[None]).reshape(-1, 3)
    lo, hi = v.min(axis=0) - 3, v.max(axis=0) + 3
    absent = np.stack([rs.randint(lo[d], hi[d] + 1, 4000) for d in range(3)], axis=1)
    absent = np.array([x for x in absent.tolist() if tuple(x) not in truth][:1000])
    assert len(absent) == 1000
    q = np.concatenate([q, absent])
    want = np.array([truth.get(tuple(x), -1) for x in q.tolist()])
    got = pr.hash_lookup(keys, vals, mask, pr.hash_key(q))
    np.testing.assert_array_equal(got, want)
    assert (got[-1000:] == -1).all() and (got[13:27 * len(v):27][present] == np.arange(len(v))[present]).all()


@pytest.fixture(scope='module')
def corner_voxels():
    a = pr.base_room(*pr.ROOM_A)
    return {name: pr.voxels(pr.placed(name, a)) for name in ('negative', 'window')}


@pytest.mark.parametrize('n,cap', [(1, 16), (7, 16), (3000, None)])
@pytest.mark.parametrize('name', ['negative', 'window'])
def test_voxel_hash_build(hip_lib, cuda_device, corner_voxels, name, n, cap):
    """Tables of 16 slots (the smallest) and of the size RegionGrower gives 3000 points, on voxels below zero on every axis and at
    the corners of the keys' window (x up to 2^20 - 1, y down to -2^20, whose neighbours fall outside it and must miss).  The
    one-point table holds a point on the x corner only; the 7-point and the 3000-point tables hold points on both."""
    v = corner_voxels[name]
    # the points on the room's largest x first, then those on its smallest y, then the rest: three of each lead the 7-point table
    on_x = np.flatnonzero(v[:, 0] == v[:, 0].max())
    on_y = np.setdiff1d(np.flatnonzero(v[:, 1] == v[:, 1].min()), on_x)
    rest = np.setdiff1d(np.arange(len(v)), np.concatenate([on_x, on_y]))
    v = v[np.concatenate([on_x[:3], on_y[:3], on_x[3:], on_y[3:], rest])][:n]
    mask = (cap or pr.hash_capacity(n)) - 1
    assert mask + 1 == (16 if cap else 8192)
    rc, keys, vals, flag = _hash_build(hip_lib, cuda_device, v, mask)
    assert (rc, flag) == (0, 0)
    if name == 'window':
        assert v[:, 0].max() == (1 << 20) - 1 and (n == 1 or v[:, 1].min() == -(1 << 20))
    _check_table(keys, vals, mask, v, np.ones(n, bool), np.random.RandomState(n))


def test_voxel_hash_build_refusals(hip_lib, cuda_device, corner_voxels):
    """The refusals, all of which return normally (the probe loop is bounded by the table size and indexes it through the mask):
    flag 1 for a voxel met twice; flag 2 for a coordinate of 2^20 or -2^20 - 1 on each axis in turn -- the other points are still
    inserted; and more points than slots (n = 20, 16 slots).  The last cannot raise flag 4 through this entry point: the call
    itself refuses a table smaller than the point count (LRG_EINVAL - 1) before it touches anything, and with at least as many slots
    as points every distinct key finds one -- flag 4 guards a condition the entry point already excludes.  Tested as that refusal."""
    from learn_region_grow_amd import _lib
    rs = np.random.RandomState(9)
    v = corner_voxels['negative'][:7].copy()
    twice = np.concatenate([v, v[2:3]])
    rc, keys, vals, flag = _hash_build(hip_lib, cuda_device, twice, 15)
    assert (rc, flag) == (0, 1)
    found = pr.hash_lookup(keys, vals, 15, pr.hash_key(v))
    assert (np.delete(found, 2) == np.delete(np.arange(7), 2)).all() and found[2] in (2, 7)
    for axis in range(3):
        for bad in (1 << 20, -(1 << 20) - 1):
            w = v.copy()
            w[4] = 0
            w[4, axis] = bad
            rc, keys, vals, flag = _hash_build(hip_lib, cuda_device, w, 15)
            assert (rc, flag) == (0, 2), (axis, bad)
            present = np.arange(7) != 4
            _check_table(keys, vals, 15, w, present, rs)
    many = corner_voxels['negative'][:20]
    rc, keys, vals, flag = _hash_build(hip_lib, cuda_device, many, 15)
    assert rc == _lib.LRG_EINVAL - 1 and flag == 0
    assert (keys.view(np.int64) == 0x1234).all() and (vals == -9).all()
    rc, keys, vals, flag = _hash_build(hip_lib, cuda_device, many, 31)          # (the smallest table that holds them)
    assert (rc, flag) == (0, 0)
    _check_table(keys, vals, 31, many, np.ones(20, bool), rs)


# =====================================================================================================
# 2. the grow loop at the placements
# =====================================================================================================
ROOM_IDS = {name: 60 + i for i, name in enumerate(sorted(pr.PLACEMENTS))}
FORMS = {'step': dict(packed=False), 'packed': dict(packed=True, free_run=False), 'graph': dict(packed=True, free_run=False, graph_iterations=4),
         'free_run': dict(free_run=True), 'hash': dict(packed=True, free_run=False)}      # 'hash': with LRG_NO_VGRID=1 (no dense grid: hash lookups)
SEEDS = range(123, 131)


@pytest.fixture(scope='module')
def parts():
    return {'a': pr.base_room(*pr.ROOM_A), 'b': pr.base_room(*pr.ROOM_B), 'small': pr.base_room(*pr.ROOM_SMALL), 'big': pr.base_room(*pr.ROOM_BIG)}


@pytest.fixture(scope='module')
def rooms(parts):
    out = {name: pr.placed(name, parts['a'], parts['b'], room_id=ROOM_IDS[name]) for name in pr.PLACEMENTS}
    for name in pr.WIDE:          # the over-wide joins again, below zero on every axis
        out[name + '@negative'] = dict(pr.place(out[name], pr.PLACEMENTS['negative'](out[name])), room_id=80 + ROOM_IDS[name])
    for key in ('small', 'big'):
        out[key] = dict(parts[key], room_id=100 + len(key))
        out[key + '@negative'] = dict(pr.place(parts[key], pr.PLACEMENTS['negative'](parts[key])), room_id=110 + len(key))
    return out


class Oracles:
    """One oracle run per (rooms, policy, set sizes of the network, restarts), shared by all formulations; policy 'net': at a seed without a near-tie
    Bernoulli draw (conftest.seed_without_near_tie)."""

    def __init__(self, rooms):
        self.rooms, self.memo = rooms, {}

    def get(self, names, policy, net, restarts=0):
        key = (tuple(names), policy, net.num_inlier_points, net.num_neighbor_points, restarts)
        if key not in self.memo:
            ni, nn = net.num_inlier_points, net.num_neighbor_points

            def run(seed):
                return [pr.oracle(self.rooms[nm], policy=policy, seed=seed, net_fn=gpu_net_fn(net), restarts=restarts, num_inlier=ni, num_neighbor=nn)
                        for nm in names]
            self.memo[key] = seed_without_near_tie(run, SEEDS, SAME_LOGITS_MARGIN) if policy == 'net' else (SEEDS[0], run(SEEDS[0]))
        return self.memo[key]


@pytest.fixture(scope='module')
def oracles(rooms):
    return Oracles(rooms)


def _grow(net, rooms, seed, policy, monkeypatch=None, form=None, in_flight=1, **kw):
    """RegionGrower(...).run(rooms) in formulation `form` (a key of FORMS) or with the arguments given; -> (grower, results)."""
    import torch
    from learn_region_grow_amd.grow import RegionGrower
    kw = dict(FORMS[form] if form else {}, rooms_in_flight=in_flight, rng='counter', seed=seed, policy=policy, **kw)
    if form == 'hash':
        monkeypatch.setenv('LRG_NO_VGRID', '1')
    if kw.get('graph_iterations'):
        with torch.cuda.stream(torch.cuda.Stream()):          # (a HIP graph is not captured on the null stream)
            gr = RegionGrower(net, **kw)
            res = gr.run(rooms)
        assert gr._graph is not None
    else:
        gr = RegionGrower(net, **kw)
        res = gr.run(rooms)
    return gr, res


def _same(got, wants):
    assert len(got) == len(wants)
    for g, w in zip(got, wants):
        same_regions(g.regions, w.regions)
        np.testing.assert_array_equal(g.cluster_label, w.cluster_label)
        np.testing.assert_array_equal(g.filled_label, w.filled_label)


KEPT = [(name, policy) for name in pr.KEEP_PVOX for policy in ('gt', 'net') if policy == 'gt' or name in pr.NET_POLICY]


@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('name,policy', KEPT)
def test_placements_with_packed_words_equal_the_oracle(net, rooms, oracles, monkeypatch, name, policy, form):
    """Every formulation -- the nine-launch step, the packed iteration, its HIP-graph replay on a side stream, the free-running
    launches, and the packed iteration on hash lookups (LRG_NO_VGRID=1) -- at every placement that keeps packed voxel words."""
    seed, wants = oracles.get([name], policy, net)
    gr, res = _grow(net, [rooms[name]], seed, policy, monkeypatch, form)
    assert gr.have_pvox
    assert gr.packed == (form != 'step') and gr.free_run == (form == 'free_run')
    if form == 'hash':
        assert gr.d_vgrid is None
    elif form != 'step':
        assert gr.d_vgrid is not None
    _same(res, wants)


@pytest.mark.parametrize('form', list(FORMS))
def test_rooms_of_different_origins_in_one_launch(net, rooms, oracles, monkeypatch, form):
    """Three rooms at different placements through two slots: the rooms of one launch have different voxel origins."""
    names = ['window', 'negative', 'fits_y']
    seed, wants = oracles.get(names, 'net', net)
    gr, res = _grow(net, [rooms[n] for n in names], seed, 'net', monkeypatch, form, in_flight=2)
    assert gr.have_pvox and gr.free_run == (form == 'free_run')
    _same(res, wants)


WIDE_ROOMS = [name + at for name in pr.WIDE for at in ('', '@negative')]
WIDE_CASES = [(name, 'gt') for name in WIDE_ROOMS] + [('wide_x', 'net'), ('wide_y@negative', 'net')]


@pytest.mark.parametrize('name,policy', WIDE_CASES)
def test_rooms_without_packed_words_equal_the_oracle(net, rooms, oracles, name, policy):
    """An extent of 2048 (x, y) or 1024 (z) voxels: no packed voxel words, so the packed iteration's front is lrg_front_kernel<7>.
    The nine-launch step, the packed iteration and the default grower (which must choose the packed iteration, lock-step) all equal
    the oracle."""
    seed, wants = oracles.get([name], policy, net)
    for kw, packed in ((dict(packed=False), False), (dict(packed=True), True), ({}, True)):
        gr, res = _grow(net, [rooms[name]], seed, policy, **kw)
        assert gr.have_pvox is False and gr.packed == packed and not gr.free_run, kw
        assert gr.d_vgrid is None
        _same(res, wants)


@pytest.mark.parametrize('name', WIDE_ROOMS)
def test_rooms_without_packed_words_refuse_free_running_launches(net, rooms, name):
    from learn_region_grow_amd.grow import RegionGrower
    with pytest.raises(ValueError):
        RegionGrower(net, rooms_in_flight=1, free_run=True).load_rooms([rooms[name]])
    assert RegionGrower.free_run_applies(net, [rooms[name]], 1) is False
    assert RegionGrower.free_run_applies(net, [rooms[name]], 1, free_run=True) is False


@pytest.mark.parametrize('name', ['fits_x', 'fits_y', 'fits_z'])
def test_preview_agrees_with_load_rooms_at_the_last_extent_that_fits(net, rooms, name):
    from learn_region_grow_amd.grow import RegionGrower
    gr = RegionGrower(net, rooms_in_flight=1).load_rooms([rooms[name]])
    assert gr.have_pvox and gr.free_run
    assert RegionGrower.free_run_applies(net, [rooms[name]], 1) == gr.free_run


def test_one_wide_room_takes_the_packed_words_from_all(net, rooms, oracles):
    """A mixed call: the ordinary room grows without packed words too, and both still equal the oracle."""
    names = ['wide_x', 'straddle']
    seed, wants = oracles.get(names, 'net', net)
    for kw in (dict(packed=True), {}):
        gr, res = _grow(net, [rooms[n] for n in names], seed, 'net', in_flight=2, **kw)
        assert gr.have_pvox is False and gr.packed and not gr.free_run
        _same(res, wants)


# =====================================================================================================
# 3. the other doors into lrg_front_kernel<7>
# =====================================================================================================
@pytest.mark.parametrize('name', ['small', 'small@negative'])
def test_restarts_with_one_slot_per_group(net, rooms, oracles, name):
    """restarts = 3 through groups of one slot: the packed iteration's front is lrg_front_kernel<7> (restarts in turn in one slot)."""
    seed, wants = oracles.get([name], 'net', net, restarts=3)
    for packed in (True, False):
        gr, res = _grow(net, [rooms[name]], seed, 'net', packed=packed, restarts=3, group_size=1)
        assert gr.have_pvox and gr.packed == packed and not gr.free_run
        _same(res, wants)
    assert max(len(r['restart_scores']) for r in wants[0].regions) == 3


@pytest.fixture(scope='module')
def net1024(cuda_device):
    return _net(cuda_device, 1024, 1024)


@pytest.mark.parametrize('name', ['big', 'big@negative'])
def test_sets_of_1024_points(net1024, rooms, oracles, name):
    """1024 + 1024 points per set (above the greedy front's 512): lrg_front_kernel<7> by set size, on a room with a region above
    1024 points under ground-truth masks, so that a set of distinct rows is full."""
    seed, wants = oracles.get([name], 'gt', net1024)
    assert max(r['points'] for r in wants[0].regions) > 1024
    for packed in (True, False):
        gr, res = _grow(net1024, [rooms[name]], seed, 'gt', packed=packed)
        assert gr.have_pvox and gr.packed == packed and not gr.free_run
        _same(res, wants)


@pytest.fixture(scope='module')
def net256(cuda_device):
    return _net(cuda_device, 256, 512)


@pytest.mark.parametrize('name', ['small', 'small@negative'])
def test_sets_of_256_and_512_points(net256, rooms, oracles, name):
    """Unequal sets below the limit, through whatever the default grower chooses."""
    net = net256
    seed, wants = oracles.get([name], 'net', net)
    gr, res = _grow(net, [rooms[name]], seed, 'net')
    assert gr.have_pvox and gr.packed
    _same(res, wants)


def test_a_voxel_outside_the_window_is_refused_and_the_grower_stays_usable(net, rooms, oracles):
    """x = 104857.6 m is voxel 2^20 at 0.1 m, one past the hash keys' window: load_rooms raises, and the same grower loads and
    grows the next room as if nothing had happened."""
    from learn_region_grow_amd._lib import LrgHipError
    from learn_region_grow_amd.grow import RegionGrower
    p = np.zeros((1, 13), np.float32)
    p[0, 0] = 104857.6
    assert int(grow_ref.voxelize(p[:, :3], pr.RES)[0, 0]) == 1 << 20
    outside = dict(points=p, obj_id=np.zeros(1, np.int32), order=np.zeros(1, np.int32), room_id=0)
    seed, wants = oracles.get(['straddle'], 'gt', net)
    gr = RegionGrower(net, rooms_in_flight=1, rng='counter', seed=seed, policy='gt')
    with pytest.raises(LrgHipError):
        gr.load_rooms([outside])
    _same(gr.run([rooms['straddle']]), wants)
