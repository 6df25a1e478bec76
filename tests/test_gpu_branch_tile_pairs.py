"""GPU: the register branch tile whose layers 0 - 2 are computed by wave pairs (csrc/lrg_wave_tile.inl: lrg_team_branch_tile_reg), as the free-running worker runs it.

A wavefront of the tile's team computes ONE 32-channel block of layers 0 - 2 and swaps it with its partner's through the team's exchange buffer (one meeting of the
two at an LDS counter per layer, the regions' writers alternating); the pooled layer's blocks alternate between two accumulators and a block's epilogue is issued
behind the next block's MFMAs.  No sum changes its order, so every value must still be the host chain's bit for bit (tests/test_gpu_wave_tile.py has the tile on a
workgroup of its own; here it runs on teams of a 512-thread workgroup that meet at LDS counters, with the kernels of two different branches at the two LDS offsets):

  `tools/wave_tile_probe.hip pairs`, run once for the three probe tests:
    single tiles   one 32-row tile per side, one and two parts; inputs under which the two blocks of a point differ in the sign of their pre-activations (the ReLU
                   of one wavefront's block must not leak into the partner's) and pooled columns that are non-positive for every point (no atomicMax);
    one pooled row two tiles of one slot: the column-wise maximum of the two host rows;
    both teams     both teams of one workgroup run 64 different tiles each, back to back: the pair counters of the two teams and of successive tiles do not meet.
  free-running labels at 4 slots (two-part register tiles) and 26 slots (one-part) against the lock-step iterations."""
import os
import re
import subprocess

import numpy as np
import pytest

from learn_region_grow_amd import synthetic
from test_gpu_grow import WEIGHT_KW, small_room, same_regions

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, 'tools', 'build', 'wave_tile_probe')


@pytest.fixture(scope='module')
def probe_out(cuda_device):
    if not os.path.exists(PROBE):      # (built by __graft_entry__.build(); here for a tree that was not)
        os.makedirs(os.path.dirname(PROBE), exist_ok=True)
        subprocess.check_call(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-I', os.path.join(ROOT, 'learn_region_grow_amd', 'csrc'),
                               os.path.join(ROOT, 'tools', 'wave_tile_probe.hip'), '-o', PROBE], stderr=subprocess.DEVNULL)
    r = subprocess.run([PROBE, 'pairs'], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode in (0, 1), r.stdout[-2000:] + r.stderr[-1000:]      # (1: values differ -- the tests below say which)
    return r.stdout


@pytest.mark.parametrize('parts', [1, 2])
def test_single_tile_per_side_equals_the_host_chain(probe_out, parts):
    m = re.search(r'single tile inputs: (\d+) of (\d+) \(point, layer\).*; (\d+) \+ (\d+) pooled columns are non-positive for every point', probe_out)
    assert m, probe_out
    assert int(m.group(1)) > 0 and int(m.group(3)) > 0 and int(m.group(4)) > 0, m.group(0)      # the inputs are what the test is about
    m = re.search(r'single tile, %d part\(s\): conv\[1\] (\d+) of (\d+) differ; layer 3 (\d+) of (\d+); pooled (\d+) of (\d+)' % parts, probe_out)
    assert m, probe_out
    assert [int(m.group(i)) for i in (2, 4, 6)] == [2 * 32 * 64, 2 * 32 * 128, 2 * 512], m.group(0)
    assert [int(m.group(i)) for i in (1, 3, 5)] == [0, 0, 0], m.group(0)


def test_two_tiles_of_a_slot_give_the_maximum_of_their_rows(probe_out):
    m = re.search(r'two tiles, one pooled row: pooled (\d+) of 512 differ .*\((\d+) columns from tile 0, (\d+) from tile 1\); conv\[1\] (\d+) differ', probe_out)
    assert m, probe_out
    assert int(m.group(2)) > 0 and int(m.group(3)) > 0, m.group(0)      # either tile decides some columns
    assert int(m.group(1)) == 0 and int(m.group(4)) == 0, m.group(0)


def test_both_teams_of_a_workgroup_run_tiles_back_to_back(probe_out):
    m = re.search(r'both teams, 64 tiles each: conv\[1\] (\d+) of (\d+) differ; layer 3 (\d+) of (\d+); pooled (\d+) of (\d+)', probe_out)
    assert m, probe_out
    assert [int(m.group(i)) for i in (2, 4, 6)] == [128 * 32 * 64, 128 * 32 * 128, 128 * 512], m.group(0)
    assert [int(m.group(i)) for i in (1, 3, 5)] == [0, 0, 0], m.group(0)


@pytest.fixture(scope='module')
def net(cuda_device):
    from learn_region_grow_amd.lrgnet import LrgNetHIP
    return LrgNetHIP(1, 1, 512, 512, 13, 0, device=cuda_device).load_weights(synthetic.make_synthetic_weights(**WEIGHT_KW))


@pytest.fixture(scope='module')
def rooms_and_lock_step(net):
    """Six generator rooms of about 1.5 k points, and what the lock-step iterations make of them (the slot count does not enter: the draws are per room)."""
    from learn_region_grow_amd.grow import RegionGrower
    rooms = [small_room(700 + i, 1400 + 50 * i, room_id=20 + i) for i in range(6)]
    want = RegionGrower(net, free_run=False, rooms_in_flight=4, rng='counter', seed=31, policy='net').run(rooms)
    return rooms, want


@pytest.mark.parametrize('in_flight', [4, 26])
def test_free_running_register_tiles_equal_lock_step(net, rooms_and_lock_step, in_flight):
    """4 slots: a branch tile is two tasks (lrg_team_branch_tile_reg<2>); 26 slots: one (<1>)."""
    from learn_region_grow_amd.grow import RegionGrower
    rooms, want = rooms_and_lock_step
    gr = RegionGrower(net, free_run=True, free_run_waves=1, rooms_in_flight=in_flight, rng='counter', seed=31, policy='net')
    got = gr.run(rooms)
    assert gr.free_run
    steps = sum(g.total_steps for g in got)
    print('%d slots: %d rooms, %d regions, %d steps' % (in_flight, len(got), sum(len(g.regions) for g in got), steps))
    assert steps >= 100      # (every step is an evaluation of ~2 x 4 branch tiles)
    for g, w in zip(got, want):
        same_regions(g.regions, w.regions)
        np.testing.assert_array_equal(g.cluster_label, w.cluster_label)
        np.testing.assert_array_equal(g.filled_label, w.filled_label)
