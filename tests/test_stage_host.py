"""CPU: the staging driver (stage_data.py) on the reference's stream, and the twin of the device teacher (tests/stage_ref.py).

The twin's loop is anchored to learn_region_grow_amd.stage.stage_room -- which the reference's own output pins
(tests/golden/stage_room150.npz, test_train_oracle.py) -- by running both on the legacy stream; the counter draws then only replace
where the random numbers come from.  The coverage checks make sure the rooms tests/test_gpu_stage.py compares on the device exercise
every path of the teacher."""
import os

import numpy as np
import pytest

import stage_ref
from conftest import GOLDEN
from learn_region_grow_amd import io as lio
from learn_region_grow_amd import preprocess, stage, synthetic

KEYS = ('points', 'remove', 'neighbor_points', 'add', 'steps', 'complete')


def assert_same_tuples(a, b):
    for k in KEYS:
        assert len(a[k]) == len(b[k]), k
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            assert np.array_equal(x, y), (k, i)


@pytest.mark.parametrize('max_points', [1024, 64])
@pytest.mark.parametrize('which', ['golden150', 'area5_1500'])
def test_twin_equals_stage_room_on_the_legacy_stream(which, max_points):
    if which == 'golden150':
        g = np.load(os.path.join(GOLDEN, 'stage_room150.npz'))
        points, obj_id = g['room_points'], g['room_obj_id']
    else:
        points, obj_id = stage_ref.prepared_room(1500, 1)
    want = stage.stage_room(points, obj_id, np.random.RandomState(0), max_points=max_points)
    got = stage_ref.stage_room_twin(points, obj_id, stage_ref.LegacyDraws(np.random.RandomState(0)), max_points=max_points)
    assert len(want['points']) > 100
    assert_same_tuples(want, got)


def test_seed_transforms():
    """stage_data.py:50-56 with Python 2's integer division: swap for 1, 3, 5, 7, then negate x for 2, 3, 6, 7, then negate y for 4 .. 7."""
    p = np.array([[1.0, 2.0, 3.0, 4.0, 5.0, 6.0], [7.0, 8.0, 9.0, 10.0, 11.0, 12.0]], dtype=np.float32)
    for seed in range(8):
        want = p.copy()
        if seed in (1, 3, 5, 7):
            want[:, 0], want[:, 1] = p[:, 1], p[:, 0]
        if seed in (2, 3, 6, 7):
            want[:, 0] = -want[:, 0]
        if seed in (4, 5, 6, 7):
            want[:, 1] = -want[:, 1]
        got = stage.seed_transform(p, seed)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got[:, 2:], p[:, 2:])
    np.testing.assert_array_equal(stage.seed_transform(p, None), p)
    assert stage.seed_transform(p, 3) is not p and p[0, 0] == 1.0            # a copy: the file's arrays stay as read


def test_file_names_follow_the_reference():
    import stage_data
    a = stage_data.parse(['--area', '1,5', '--data-dir', 'd'])
    assert [stage_data.input_path(a, x) for x in a.areas] == [os.path.join('d', 's3dis_area1.h5'), os.path.join('d', 's3dis_area5.h5')]
    assert stage_data.output_path(a, '5') == os.path.join('d', 'staged_area5.h5')
    a = stage_data.parse(['--area', 'scannet,kitti_train,synthetic_test', '--seed', '3', '--data-dir', 'd'])
    assert stage_data.input_path(a, 'scannet') == os.path.join('d', 'scannet.h5')
    assert stage_data.input_path(a, 'kitti_train') == os.path.join('d', 'kitti_train_03.h5')
    assert stage_data.output_path(a, 'scannet') == os.path.join('d', 'multiseed', 'seed3_areascannet.h5')
    assert stage_data.output_path(a, 'synthetic_test') == os.path.join('d', 'staged_synthetic_test.h5')
    assert a.rng == 'counter' and a.preprocess == 'gpu-exact' and a.max_points == 1024
    for bad in (['--area', 'kitti_train'], ['--area', '9'], ['--area', '1,2', '--out', 'x.h5']):
        with pytest.raises(SystemExit):
            stage_data.parse(bad)


def test_driver_on_the_legacy_stream_without_a_gpu(tmp_path, capsys):
    """stage_data.py --rng legacy --preprocess host on a two-room file: the reference's file name, and the tuples of stage_room with ONE
    stream running across both rooms."""
    import stage_data
    raw = [synthetic.area5_shaped_room(600, seed=5).astype(np.float32), synthetic.area5_shaped_room(500, seed=6).astype(np.float32)]
    lio.saveToH5(str(tmp_path / 'synthetic_unit.h5'), raw)
    stage_data.main(['--area', 'synthetic_unit', '--data-dir', str(tmp_path), '--rng', 'legacy', '--preprocess', 'host'])
    lines = capsys.readouterr().out.splitlines()
    assert any(x.startswith('AREA synthetic_unit room 0 target ') for x in lines) and any(x.startswith('AREA synthetic_unit room 1 target ') for x in lines)
    path = tmp_path / 'staged_synthetic_unit.h5'
    assert path.exists()
    got = stage.load_staged(str(path))
    rs = np.random.RandomState(0)
    parts = []
    for r in raw:
        p = preprocess.preprocess_room(r[:, :6], r[:, 6].astype(int), r[:, 7].astype(int))
        parts.append(stage.stage_room(p['points'], p['obj_id'], rs))
    want = stage.center_tuples(stage.merge(parts))
    assert len(parts[0]['points']) > 0 and len(parts[1]['points']) > 0
    for k in ('points', 'remove', 'neighbor_points', 'add'):
        assert len(got[k]) == len(want[k])
        assert all(np.array_equal(x, y) for x, y in zip(got[k], want[k])), k
    # one stream across both rooms: the second room staged on a stream of its own gives other tuples
    p1 = preprocess.preprocess_room(raw[1][:, :6], raw[1][:, 6].astype(int), raw[1][:, 7].astype(int))
    alone = stage.stage_room(p1['points'], p1['obj_id'], np.random.RandomState(0))
    assert [len(x) for x in alone['points']] != [len(x) for x in parts[1]['points']]


def test_gpu_rooms_cover_every_path_of_the_teacher():
    """What tests/test_gpu_stage.py compares on the device is not vacuous: under the counter draws of those tests ..."""
    rooms = stage_ref.gpu_rooms()
    assert [len(r['points']) for r in rooms][1:3] == [1, 63] and len(set(rooms[3]['obj_id'])) == 1 and len(rooms[3]['points']) > 100 and [r['room_id'] for r in rooms] == list(stage_ref.ROOM_IDS)
    max_iters = 2 * 500 + 64
    # ... at max_points = 64 on the 1500-point room both sides are subsampled, objects complete, small ones are dropped, odd and even counts occur
    st, stats = stage_ref.twin(0, max_points=64)
    assert stats['sub_in'] > 100 and stats['sub_nb'] > 100
    assert stats['completed'] > 10 and stats['stored'] > 10 and stats['small_dropped'] > 0
    counts = np.array([len(p) for p in st['points']])
    assert (counts % 2 == 1).sum() > 10 and (counts % 2 == 0).sum() > 10 and counts.max() == 64
    assert max(stats['passes']) <= max_iters // 4
    # ... the same room at 1024 emits whole sides of odd and even counts
    st, stats = stage_ref.twin(0)
    counts = np.array([len(p) for p in st['points']])
    assert (counts % 2 == 1).sum() > 10 and (counts % 2 == 0).sum() > 10 and stats['sub_in'] == 0
    # ... the one-point room: one object, one pass, nothing emitted, nothing stored
    st, stats = stage_ref.twin(1)
    assert stats['passes'] == [1] and len(st['points']) == 0 and st['steps'] == [0]
    # ... the room that is all one object: its last pass completes with an empty neighbourhood and emits nothing
    st, stats = stage_ref.twin(3)
    assert stats['completed'] == 1 and stats['stored'] == 1 and len(st['steps']) == 1
    assert stats['passes'][0] == st['steps'][0] + 1 and len(st['points']) == st['steps'][0] > 3
    # ... the 6000-point room reaches the full inlier side of 1024 and subsamples it
    st, stats = stage_ref.twin(4)
    assert stats['max_in'] == 1024 and stats['sub_in'] > 0 and stats['sub_nb'] > 0
    assert max(stats['passes']) <= max_iters // 4


def test_twin_raises_at_the_iteration_cap():
    points, obj_id = stage_ref.gpu_rooms()[3]['points'], stage_ref.gpu_rooms()[3]['obj_id']
    with pytest.raises(stage_ref.IterCap):
        stage_ref.stage_room_twin(points, obj_id, stage_ref.CounterDraws(stage_ref.RNG_SEED, 20), max_iters=3)
