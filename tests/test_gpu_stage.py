"""GPU: the device teacher (lrg_stage_teacher / lrg_stage_tuples, stage.stage_rooms_gpu) against its host twin (tests/stage_ref.py under
CounterDraws), byte for byte: the outputs are integer decisions, float32 subtractions and exact medians, so there is no tolerance.
tests/test_stage_host.py anchors the twin to the reference and shows that these rooms exercise every path."""
import glob
import os

import numpy as np
import pytest

import stage_ref
from learn_region_grow_amd import io as lio
from learn_region_grow_amd import h5lite, stage, synthetic

pytestmark = pytest.mark.gpu


def staged_bytes(st):
    """The eight datasets of a staged file as save_staged lays them out."""
    return dict(points=np.vstack(st['points']).astype(np.float32).tobytes() if st['points'] else b'',
                count=np.array([len(p) for p in st['points']], dtype=np.int32).tobytes(),
                remove=np.concatenate(st['remove']).astype(np.int32).tobytes() if st['remove'] else b'',
                neighbor_points=np.vstack(st['neighbor_points']).astype(np.float32).tobytes() if st['neighbor_points'] else b'',
                neighbor_count=np.array([len(p) for p in st['neighbor_points']], dtype=np.int32).tobytes(),
                add=np.concatenate(st['add']).astype(np.int32).tobytes() if st['add'] else b'',
                steps=np.array(st['steps'], dtype=np.int32).tobytes(),
                complete=np.array(st['complete'], dtype=np.float32).tobytes())


def assert_same_bytes(got, want):
    g, w = staged_bytes(got), staged_bytes(want)
    for k in ('count', 'neighbor_count', 'steps', 'complete', 'remove', 'add', 'points', 'neighbor_points'):
        assert len(g[k]) == len(w[k]), k
        assert g[k] == w[k], k


def twin_of(indices, max_points=1024):
    return stage_ref.center(stage.merge([stage_ref.twin(i, max_points)[0] for i in indices]))


@pytest.fixture(scope='module')
def five_rooms(cuda_device):
    info = {}
    st = stage.stage_rooms_gpu(stage_ref.gpu_rooms(), seed=stage_ref.RNG_SEED, device=cuda_device, info=info)
    return st, info


def test_five_rooms_in_one_launch(five_rooms):
    st, info = five_rooms
    assert info['launches'] == 1 and info['overflowed'] == []
    want = twin_of(range(5))
    assert len(want['points']) > 2000 and max(len(p) for p in want['points']) == 1024
    assert_same_bytes(st, want)
    # per room: the stored objects' step counts
    for i in range(5):
        assert [int(x) for x in info['objects'][i][:, 0]] == stage_ref.twin(i)[0]['steps']


def test_subsampled_sides_at_64_points(cuda_device):
    st = stage.stage_rooms_gpu(stage_ref.gpu_rooms()[:1], seed=stage_ref.RNG_SEED, max_points=64, device=cuda_device)
    assert_same_bytes(st, twin_of([0], max_points=64))


def test_overflow_relaunch_gives_the_roomy_result(cuda_device, five_rooms):
    info = {}
    st = stage.stage_rooms_gpu(stage_ref.gpu_rooms(), seed=stage_ref.RNG_SEED, device=cuda_device, arena_entries=256, info=info)
    assert info['launches'] > 1
    assert {0, 3, 4} <= set(info['overflowed']) and 1 not in info['overflowed']      # the one-point room emits nothing
    assert_same_bytes(st, five_rooms[0])


def test_two_launches_give_the_same_bytes(cuda_device, five_rooms):
    again = stage.stage_rooms_gpu(stage_ref.gpu_rooms(), seed=stage_ref.RNG_SEED, device=cuda_device)
    assert_same_bytes(again, five_rooms[0])


def test_another_seed_gives_another_seed_order(cuda_device, five_rooms):
    info = {}
    stage.stage_rooms_gpu(stage_ref.gpu_rooms()[:1], seed=stage_ref.RNG_SEED + 1, device=cuda_device, info=info)
    first = five_rooms[1]['objects'][0][:, 1]
    other = info['objects'][0][:, 1]
    assert len(first) > 10 and len(other) > 10 and list(first[:10]) != list(other[:10])
    assert [int(x) for x in info['objects'][0][:, 0]] == stage_ref.twin(0, seed=stage_ref.RNG_SEED + 1)[0]['steps']


def test_limits_are_refused(cuda_device):
    with pytest.raises(ValueError):
        stage.stage_rooms_gpu(stage_ref.gpu_rooms()[1:2], max_points=2048, device=cuda_device)
    from learn_region_grow_amd import _lib
    with pytest.raises(_lib.LrgHipError, match='room_id 20'):
        stage.stage_rooms_gpu(stage_ref.gpu_rooms()[3:4], seed=stage_ref.RNG_SEED, max_iters=3, device=cuda_device)


def test_driver_then_training(cuda_device, tmp_path, capsys):
    """stage_data.py --rng counter on a synthetic file, then one epoch of train_region_grow.py on what it wrote."""
    import stage_data
    import train_region_grow
    raw = [synthetic.area5_shaped_room(600, seed=5).astype(np.float32), synthetic.area5_shaped_room(500, seed=6).astype(np.float32)]
    lio.saveToH5(str(tmp_path / 'synthetic_unit.h5'), raw)
    stage_data.main(['--area', 'synthetic_unit', '--data-dir', str(tmp_path), '--rng', 'counter', '--max-points', '512'])
    out = capsys.readouterr().out
    assert 'AREA synthetic_unit room 1 target ' in out
    staged = str(tmp_path / 'staged_synthetic_unit.h5')
    data = stage.load_staged(staged)
    assert len(data['points']) >= 8 and data['points'][0].shape[1] == 13
    assert len(h5lite.File(staged)['steps'].read()) > 10              # stored objects
    prefix = str(tmp_path / 'models' / 'lrgnet_unit.ckpt')
    assert train_region_grow.main(['--staged', staged, '--epochs', '1', '--batch-size', '4', '--ckpt', prefix]) == 0
    out = capsys.readouterr().out
    line = [x for x in out.splitlines() if x.startswith('Epoch 0 loss ')]
    assert line and np.isfinite(float(line[0].split()[3]))
    assert glob.glob(prefix + '*'), os.listdir(os.path.dirname(prefix))
