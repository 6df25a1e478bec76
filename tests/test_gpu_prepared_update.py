"""GPU: the prepared mask update of the free-running launches (csrc/lrg_front.inl, LrgPrepRecord): the part of a slot's update that does not depend on
the evaluation in flight is worked out while that evaluation runs and kept in the front workgroup's LDS; the update behind the arrival reads the logits
and the record.  The lock-step iterations and the oracle have no record, so every comparison here is prepared against unprepared: regions, cluster
labels and filled labels must be equal exactly -- with records that are never valid (one step per launch), valid for one step, and mixed; with one, two
and three slots per front workgroup (the third has no record); with launches so short that slots leave and re-enter them; with regions larger than a
record's list; and in a room built so that taken points do change voxel on the float32 round trip through the centre (a valid record, and the step
takes the general form all the same)."""
import numpy as np
import pytest

from learn_region_grow_amd import synthetic, workloads
from oracle import grow_ref, rng_ref
from test_gpu_grow import WEIGHT_KW, small_room, same_regions
from test_gpu_fullsize import zero_net

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def net(cuda_device):
    from learn_region_grow_amd.lrgnet import LrgNetHIP
    return LrgNetHIP(1, 1, 512, 512, 13, 0, device=cuda_device).load_weights(synthetic.make_synthetic_weights(**WEIGHT_KW))


def _rooms():
    return [small_room(400 + i, 600 + 200 * i, room_id=10 + i) for i in range(3)] + \
           [small_room(300, 1500, furniture=4, room_id=13), small_room(301, 2500, furniture=6, room_id=14), small_room(403, 900, room_id=15)]


KW = dict(rooms_in_flight=6, rng='counter', seed=123, policy='net')


@pytest.fixture(scope='module')
def lock_step(net):
    from learn_region_grow_amd.grow import RegionGrower
    return RegionGrower(net, free_run=False, **KW).run(_rooms())


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        same_regions(g.regions, w.regions)
        np.testing.assert_array_equal(g.cluster_label, w.cluster_label)
        np.testing.assert_array_equal(g.filled_label, w.filled_label)


@pytest.mark.parametrize('waves', [1, -1])
@pytest.mark.parametrize('steps,fronts', [(1, 6), (2, 6), (2, 3), (7, 3), (7, 2), (64, 6), (64, 3), (64, 2)])
def test_prepared_update_equals_lock_step(net, lock_step, steps, fronts, waves):
    """steps per slot and launch: 1 = no record is ever valid (LDS does not outlive a launch), 2 = valid for one step, 7 / 64 = mixed.  fronts: six
    slots on 6 / 3 / 2 front workgroups = one / two / three slots per workgroup (the third without a record).  waves: 1 = register tiles, -1 = the
    one-kernel launch."""
    from learn_region_grow_amd.grow import RegionGrower
    gr = RegionGrower(net, free_run=True, free_run_steps=steps, free_run_fronts=fronts, free_run_waves=waves, **KW)
    got = gr.run(_rooms())
    assert gr.free_run
    _same(got, lock_step)


@pytest.mark.parametrize('waves,fronts', [(1, 3), (-1, 3), (1, 2)])
def test_short_launches(net, lock_step, waves, fronts):
    """Launches of 1.5 ms: slots leave and re-enter launches with shared tail rows in use (a record never survives the launch it was made in)."""
    from learn_region_grow_amd.grow import RegionGrower
    gr = RegionGrower(net, free_run=True, free_run_budget_us=1500, free_run_fronts=fronts, free_run_waves=waves, **KW)
    _same(gr.run(_rooms()), lock_step)


def test_regions_above_the_record_list(net):
    """The 45 k-point room of the Area-5-shaped set under ground-truth masks: regions above 2048 members (no record: the list would not fit) and above 4096
    (the update's second pass over the list), between steps that are prepared."""
    from learn_region_grow_amd.grow import RegionGrower
    big = workloads.make_room(45063, 1057, 57)
    kw = dict(rooms_in_flight=1, rng='counter', seed=5, policy='gt')
    want = RegionGrower(net, free_run=False, **kw).run([big])
    gr = RegionGrower(net, free_run=True, **kw)
    got = gr.run([big])
    assert gr.free_run
    sizes = [r['points'] for r in want[0].regions]
    assert max(sizes) > 4096 and min(sizes) <= 2048
    _same(got, want)


def edge_room():
    """small_room(301, 2500, furniture=6) with x and y of every 8th point replaced by the largest float32 that still rounds to the point's own voxel: the
    voxels -- and with them the equalisation -- are unchanged, and (x - c) + c in float32 carries many of these points over the voxel boundary."""
    room = small_room(301, 2500, furniture=6, room_id=14)
    pts = room['points'].copy()
    res = np.float32(0.1)
    vox = grow_ref.voxelize(pts[:, :3], 0.1)
    for d in (0, 1):
        v = vox[::8, d]
        x = ((v + 0.5) * 0.1).astype(np.float32)
        for _ in range(64):
            off = np.round(x / res).astype(np.int64) != v
            if not off.any():
                break
            x[off] = np.nextafter(x[off], np.float32(-np.inf))
        assert not off.any()
        pts[::8, d] = x
    np.testing.assert_array_equal(grow_ref.voxelize(pts[:, :3], 0.1), vox)
    room['points'] = pts
    return room


def count_moved(room, steps):
    """(steps with at least one taken row whose re-derived voxel (:271-276) is not its point's own, steps without one, such rows, taken rows), from the
    oracle hook's records."""
    pv = grow_ref.voxelize(room['points'][:, :3], 0.1)
    with_moved = without = rows_moved = rows_taken = 0
    for h in steps:
        members = np.flatnonzero(h['mask_before'])
        box = np.all(pv >= h['min_dims'] - 1, axis=1) & np.all(pv <= h['max_dims'] + 1, axis=1)
        cands = np.flatnonzero(box & ~h['mask_before'] & ~h['visited'])
        assert len(members) == h['nc'] and len(cands) == h['ne']
        moved = 0
        for rows, mask, own in ((h['neighbor'][0], h['add_mask'], cands[h['subset_nb']]), (h['inlier'][0], h['rmv_mask'], members[h['subset_in']])):
            q = rows[mask][:, :3].copy()
            q[:, :2] += h['center'][:2]
            moved += int(np.any(grow_ref.voxelize(q, 0.1) != pv[own[mask]], axis=1).sum())
            rows_taken += int(mask.sum())
        rows_moved += moved
        if moved:
            with_moved += 1
        else:
            without += 1
    return with_moved, without, rows_moved, rows_taken


def test_moved_voxels_take_the_general_form(net):
    """A valid record whose step must not use it: taken points that change voxel on the round trip through the centre.  The room is checked first (both
    kinds of step occur in it, interleaved, under ground-truth masks: the count does not depend on any network), then free-running == lock-step ==
    oracle under ground-truth masks and free-running == lock-step under the Bernoulli policy."""
    from learn_region_grow_amd.grow import RegionGrower
    room = edge_room()
    steps = []
    want = grow_ref.grow_room(room['points'], room['obj_id'], room['order'], None, rng_ref.CounterStream(123, room['room_id']),
                              net_fn=zero_net, policy='gt', hook=steps.append)
    with_moved, without, rows_moved, rows_taken = count_moved(room, steps)
    print('steps %d: %d with a moved voxel (%d of %d taken rows), %d without' % (len(steps), with_moved, rows_moved, rows_taken, without))
    assert with_moved > 0 and without > 0
    kw = dict(rooms_in_flight=1, rng='counter', seed=123)
    lock = RegionGrower(net, free_run=False, policy='gt', **kw).run([room])
    gr = RegionGrower(net, free_run=True, policy='gt', **kw)
    free = gr.run([room])
    assert gr.free_run
    _same(free, lock)
    _same(free, [want])
    lock = RegionGrower(net, free_run=False, policy='net', **kw).run([room])
    free = RegionGrower(net, free_run=True, policy='net', **kw).run([room])
    _same(free, lock)


def test_speculation_sees_no_record(net):
    """Three regions per room in flight on 16 rooms: the speculating front step has no prepared form and must not meet a record."""
    from learn_region_grow_amd.grow import RegionGrower
    rooms = [small_room(500 + i, 500 + 60 * i, room_id=30 + i) for i in range(16)]
    kw = dict(rooms_in_flight=16, rng='counter', seed=9, policy='net')
    want = RegionGrower(net, free_run=True, **kw).run(rooms)
    gr = RegionGrower(net, speculate=3, **kw)
    got = gr.run(rooms)
    assert gr.free_run and gr.speculate == 3
    _same(got, want)
