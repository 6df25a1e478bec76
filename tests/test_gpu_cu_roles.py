"""GPU: register-tile CUs by role (csrc/lrg_async_plan.h: lrg_rt_role; LRG_ASYNC_RT_HEAD_EVERY) -- branch tiles alone on their CUs, head tiles on CUs of their own.

With the switch at N, one worker CU in N of every XCD's share runs head tiles on BOTH its teams (HEAD2: no branch kernels in LDS, the second head team's region
in their place) and the others run branch tiles on team 0 alone (BRANCH1: team 1's wavefronts leave at the start).  Only who takes which ring's tickets changes:
every label, region log and logit must stay what it was.

  `tools/wave_tile_probe.hip roles`: both head teams of one workgroup run 64 different head tiles each, back to back, on the HEAD2 layout of the LDS -- and the
      other three pairings the probe times (a head tile alone, beside a branch team, a branch tile with team 1 absent): every value is the host chain's bit for bit;
  free-running labels, region logs and filled labels against the lock-step iterations at 4, 26 and 68 slots in flight with the switch forced to 2 and to 3, and at
      68 slots with the switch unset (the default plan); two runs of one case give the same labels."""
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
SWITCH = 'LRG_ASYNC_RT_HEAD_EVERY'


@pytest.fixture(scope='module')
def probe_out(cuda_device):
    src = os.path.join(ROOT, 'tools', 'wave_tile_probe.hip')
    if not os.path.exists(PROBE) or os.path.getmtime(PROBE) < os.path.getmtime(src):      # (built by __graft_entry__.build(); here for a tree that was not)
        os.makedirs(os.path.dirname(PROBE), exist_ok=True)
        subprocess.check_call(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-I', os.path.join(ROOT, 'learn_region_grow_amd', 'csrc'),
                               src, '-o', PROBE], stderr=subprocess.DEVNULL)
    r = subprocess.run([PROBE, 'roles'], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode in (0, 1), r.stdout[-2000:] + r.stderr[-1000:]      # (1: values differ -- the tests below say which)
    return r.stdout


def roles_line(out, name):
    m = re.search(r'roles %s, 64 tiles per team: logits (\d+) of (\d+) differ from the host chain; conv\[1\] (\d+) of (\d+); pooled (\d+) of (\d+)' % re.escape(name), out)
    assert m, out
    return [int(v) for v in m.groups()]


def test_two_head_teams_of_a_workgroup_run_tiles_back_to_back(probe_out):
    """The HEAD2 layout: team 0's head region where the branch kernels would lie, team 1's in its usual place; 2 x 64 tiles of 32 rows x 2 logits."""
    bad_l, n_l, bad_c, n_c, bad_p, n_p = roles_line(probe_out, '(b) a head tile beside a head team')
    assert (n_l, n_c, n_p) == (2 * 64 * 32 * 2, 0, 0)
    assert bad_l == 0


@pytest.mark.parametrize('name,counts', [('(a) a head tile alone', (64 * 64, 0, 0)),
                                         ('(c) a head tile beside a branch team', (64 * 64, 64 * 32 * 64, 64 * 512)),
                                         ('(d) a branch tile, team 1 absent', (0, 64 * 32 * 64, 64 * 512))])
def test_the_other_pairings_equal_the_host_chain(probe_out, name, counts):
    bad_l, n_l, bad_c, n_c, bad_p, n_p = roles_line(probe_out, name)
    assert (n_l, n_c, n_p) == counts
    assert (bad_l, bad_c, bad_p) == (0, 0, 0)


def test_probe_times_the_four_pairings(probe_out):
    """(the figures themselves: profiles/cu_roles.txt)"""
    ticks = re.findall(r'ROLES \((a|b|c|d)\) [^\n]*, grid +(1|200): +(\d+) counter ticks per tile', probe_out)
    assert sorted((k, int(g)) for k, g, _ in ticks) == [(k, g) for k in 'abcd' for g in (1, 200)], probe_out
    assert all(int(v) > 0 for _, _, v in ticks)


@pytest.fixture(scope='module')
def net(cuda_device):
    from learn_region_grow_amd.lrgnet import LrgNetHIP
    return LrgNetHIP(1, 1, 512, 512, 13, 0, device=cuda_device).load_weights(synthetic.make_synthetic_weights(**WEIGHT_KW))


@pytest.fixture(scope='module')
def rooms_and_lock_step(net):
    """The six generator rooms of about 1.5 k points of tests/test_gpu_branch_tile_pairs.py, and what the lock-step iterations make of them (computed once)."""
    from learn_region_grow_amd.grow import RegionGrower
    rooms = [small_room(700 + i, 1400 + 50 * i, room_id=20 + i) for i in range(6)]
    want = RegionGrower(net, free_run=False, rooms_in_flight=4, rng='counter', seed=31, policy='net').run(rooms)
    return rooms, want


def free_run(net, rooms, in_flight):
    from learn_region_grow_amd.grow import RegionGrower
    gr = RegionGrower(net, free_run=True, free_run_waves=1, rooms_in_flight=in_flight, rng='counter', seed=31, policy='net')
    got = gr.run(rooms)
    assert gr.free_run
    return got


@pytest.mark.parametrize('in_flight,head_every', [(4, 2), (4, 3), (26, 2), (26, 3), (68, 2), (68, 3), (68, None)])
def test_free_running_labels_by_role_equal_lock_step(net, rooms_and_lock_step, monkeypatch, in_flight, head_every):
    """(the switches are read on every call of the launch; None: the switch unset -- the plan's own choice)"""
    rooms, want = rooms_and_lock_step
    if head_every is None:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, str(head_every))
    got = free_run(net, rooms, in_flight)
    steps = sum(g.total_steps for g in got)
    print('%d slots, %s=%s: %d rooms, %d regions, %d steps' % (in_flight, SWITCH, head_every, len(got), sum(len(g.regions) for g in got), steps))
    assert steps >= 100
    for g, w in zip(got, want):
        same_regions(g.regions, w.regions)
        np.testing.assert_array_equal(g.cluster_label, w.cluster_label)
        np.testing.assert_array_equal(g.filled_label, w.filled_label)


def test_two_runs_give_the_same_labels(net, rooms_and_lock_step, monkeypatch):
    rooms, _ = rooms_and_lock_step
    monkeypatch.setenv(SWITCH, '3')
    first, second = free_run(net, rooms, 26), free_run(net, rooms, 26)
    for a, b in zip(first, second):
        np.testing.assert_array_equal(a.cluster_label, b.cluster_label)
        np.testing.assert_array_equal(a.filled_label, b.filled_label)
