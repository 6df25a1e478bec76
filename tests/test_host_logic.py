"""CPU: host-side decisions of the round-5 features (no GPU, no library calls that compute)."""
import numpy as np
import pytest


class _Net:           # what RegionGrower.free_run_applies looks at
    mode = 'fused'
    num_inlier_points = 512
    num_neighbor_points = 512
    lite = 0


def _room(n, extent=5.0, seed=0):
    rs = np.random.RandomState(seed)
    p = np.zeros((n, 13), np.float32)
    p[:, :3] = rs.rand(n, 3) * extent
    return dict(points=p, obj_id=np.zeros(n, np.int32), order=np.arange(n, dtype=np.int32))


def test_auto_speculate_by_rooms_per_gpu():
    from learn_region_grow_amd.grow import auto_speculate
    assert [auto_speculate(n) for n in (1, 8, 16, 17, 32, 33, 68, 272)] == [3, 3, 3, 2, 2, 0, 0, 0]


def test_free_run_applies_matches_the_growers_rules():
    from learn_region_grow_amd import _lib
    from learn_region_grow_amd.grow import RegionGrower
    net = _Net()
    rooms = [_room(2000), _room(3000, seed=1)]
    assert RegionGrower.free_run_applies(net, rooms, 68)
    assert not RegionGrower.free_run_applies(net, rooms, 68, free_run=False)
    assert not RegionGrower.free_run_applies(net, rooms, 68, restarts=16)                      # restarts: lock-step groups
    assert not RegionGrower.free_run_applies(net, rooms, 68, rng='legacy')
    assert not RegionGrower.free_run_applies(net, rooms, 68, packed=False)
    assert not RegionGrower.free_run_applies(net, rooms, _lib.LRG_FREE_RUN_AUTO_SLOTS + 1)     # hundreds of slots: lock-step by default ...
    assert RegionGrower.free_run_applies(net, rooms, _lib.LRG_FREE_RUN_AUTO_SLOTS + 1, free_run=True)      # ... unless asked for
    far = _room(100, extent=250.0)                       # 2 500 voxels across at 0.1 m: no packed voxel words (2048 x 2048 x 1024 at most)
    assert not RegionGrower.free_run_applies(net, [far], 4)
    assert RegionGrower.free_run_applies(net, [far], 4, resolution=0.3)
    lite1 = _Net(); lite1.lite = 1
    assert not RegionGrower.free_run_applies(lite1, rooms, 68)
    assert not RegionGrower.free_run_applies(net, [], 68)


def test_choose_formulation_table():
    """The one rule behind RegionGrower.load_rooms, free_run_applies and LanedRegionGrower's lanes: (packed, free_run) for each
    change of the facts of 68 greedy slots over two small rooms, or the ValueError of a wish the facts rule out."""
    from learn_region_grow_amd import _lib
    from learn_region_grow_amd.grow import choose_formulation
    base = dict(mode='fused', lite=0, n_inlier=512, n_neighbor=512, room_points=[2000, 3000], have_pvox=True, S=68, G=1, restarts=1,
                rng='counter', packed=None, free_run=None, skip_duplicate_rows=True, speculate=0, packed_workspace=True, env_free_run=True)
    big = _lib.LRG_PACKED_MAX_POINTS + 1
    table = [({}, (True, True)),
             (dict(free_run=False), (True, False)),
             (dict(env_free_run=False), (True, False)),                                     # LRG_FREE_RUN=0: lock-step by default ...
             (dict(env_free_run=False, free_run=True), (True, True)),                       # ... unless asked for
             (dict(S=_lib.LRG_FREE_RUN_AUTO_SLOTS + 1), (True, False)),
             (dict(S=_lib.LRG_FREE_RUN_AUTO_SLOTS + 1, free_run=True), (True, True)),
             (dict(packed=False), (False, False)),
             (dict(packed=False, free_run=True), (False, False)),                           # (not refused: no packed iterations, no free run)
             (dict(packed=True), (True, True)),
             (dict(restarts=16, G=16, S=68 * 16), (True, False)),
             (dict(speculate=3, G=3, S=204, free_run=True), (True, True)),
             (dict(have_pvox=False), (True, False)),
             (dict(lite=1), (True, False)),
             (dict(lite=2), (True, True)),
             (dict(n_inlier=1024), (True, False)),
             (dict(n_neighbor=2048), (False, False)),
             (dict(room_points=[big]), (False, False)),
             (dict(room_points=[]), (True, True)),                                          # no rooms known yet
             (dict(mode='streamed'), (False, False)),
             (dict(rng='legacy', skip_duplicate_rows=False), (False, False)),
             (dict(skip_duplicate_rows=False), (False, False)),
             (dict(packed_workspace=False), (False, False)),
             (dict(mode='streamed', free_run=True), 'free-running launches need packed iterations'),
             (dict(packed_workspace=False, free_run=True, packed=True), 'free-running launches need packed iterations'),
             (dict(mode='streamed', packed=True), 'packed iterations need the counter stream'),
             (dict(room_points=[big], packed=True), 'packed iterations need the counter stream'),
             (dict(restarts=16, G=16, free_run=True), 'free-running launches need greedy growing'),
             (dict(have_pvox=False, free_run=True), 'free-running launches need greedy growing'),
             (dict(lite=1, free_run=True), 'free-running launches need greedy growing'),
             (dict(n_inlier=1024, free_run=True), 'free-running launches need greedy growing')]
    for change, want in table:
        facts = dict(base, **change)
        if isinstance(want, str):
            with pytest.raises(ValueError, match=want):
                choose_formulation(**facts)
        else:
            assert choose_formulation(**facts) == want, change


def test_speculate_argument_checks():
    from learn_region_grow_amd.grow import RegionGrower
    with pytest.raises(ValueError):
        RegionGrower(_Net(), speculate=3, restarts=4)
    with pytest.raises(ValueError):
        RegionGrower(_Net(), speculate=3, free_run=False)
    with pytest.raises(ValueError):
        RegionGrower(_Net(), speculate=17)


def test_lanes_refuse_free_running_side_by_side():
    from learn_region_grow_amd.grow import LanedRegionGrower
    with pytest.raises(ValueError):
        LanedRegionGrower(_Net(), rooms_in_flight=8, lanes=2, free_run=True)


def test_tail_and_queue_bytes_are_host_arithmetic(hip_lib):
    assert hip_lib.lrg_grow_async_tail_bytes(0, 4096) == 0 and hip_lib.lrg_grow_async_tail_bytes(68, 100) == 0      # (rows: a multiple of 32)
    assert hip_lib.lrg_grow_async_tail_bytes(68, 4096) == 4 * (32 + 4 * 128 + 2 * 68)
    assert hip_lib.lrg_grow_async_queue_bytes(68) > 0


def test_bench_arguments():
    import bench
    import sys
    old = sys.argv
    try:
        sys.argv = ['bench.py']
        a = bench.parse()
        assert a.speculate == -1 and a.one_room_ks == '1,2,3,4,6' and a.one_rank_collective == 1 and '320' in a.best_slots
    finally:
        sys.argv = old


def test_bench_area5_rooms_side_by_side_are_the_set(tmp_path):
    """bench.py generates the Area-5 set in processes side by side (start_area5_rooms, the largest rooms first): the rooms of
    workloads.area5_rooms in its order, bit for bit -- generated and cached, then read back from the cache."""
    import bench
    from learn_region_grow_amd import workloads
    want = workloads.area5_rooms(3, seed_base=1000)
    for _ in range(2):
        got = bench.start_area5_rooms(3, 1000, str(tmp_path), 2)()
        assert len(got) == 3
        for a, b in zip(got, want):
            assert a['room_id'] == b['room_id']
            for k in ('points', 'obj_id', 'order'):
                assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
