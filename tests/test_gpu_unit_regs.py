"""GPU: the pooled-product units with their slice in registers (csrc/lrg_async_units.inl: lrg_async_gemv_unit3; plan field unit_regs, switch LRG_ASYNC_UNIT_REGS).

Eight engine wavefronts keep a [1024, 32] slice of a head's first-layer kernel in registers, four fetchers stream the slots' pooled rows through an LDS FIFO and
four writers sum up, store and arrive.  What goes into a unit and what comes out of it is what it was, and so is the summation order: every label, region log and
logit must stay what it was.

  `tools/wave_tile_probe.hip units`: each of the three unit forms alone on hand-made rows and ring entries -- every sum is the host chain's bit for bit, with
      pooled rows and with per-tile pool rows (slots whose sides have 1 .. 16 tiles); the latency and capacity figures: profiles/unit_registers.txt;
  free-running labels, region logs and filled labels against the lock-step iterations at 4, 26, 68 and 100 slots with the form forced on; at 68 slots with the
      switch unset (what the plan chose is asserted through lrg_async_last_plan); with launches of 1.5 ms (the units leave and come back a few hundred times); with
      rooms that run out in the middle of a launch; two runs of one case alike; one audit of every step at 68 slots, logits bit for bit; lite 2 at 84 slots, which
      must keep the four-team form."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import step_audit as sa
from conftest import seed_without_near_tie
from learn_region_grow_amd import synthetic
from test_gpu_grow import WEIGHT_KW, SAME_LOGITS_MARGIN, gpu_net_fn, small_room, same_regions

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, 'tools', 'build', 'wave_tile_probe')
SWITCH = 'LRG_ASYNC_UNIT_REGS'
SEED = 31
PLAN_WORDS = ['planned', 'two_kernels', 'front_wgs', 'worker_wgs', 'n_front', 'gemv_units', 'unit_pairs', 'unit_regs', 'reg_tiles', 'teams', 'pool_rows', 'n_slots']


def last_plan():
    """What the process's last lrg_grow_async planned (csrc/lrg_async_plan.h: lrg_async_last_plan; not part of include/lrg_hip.h)."""
    from learn_region_grow_amd import _lib
    fn = ctypes.CDLL(_lib.LIB_PATH).lrg_async_last_plan
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
    out = (ctypes.c_int32 * len(PLAN_WORDS))()
    assert fn(out, len(PLAN_WORDS)) == len(PLAN_WORDS)
    plan = dict(zip(PLAN_WORDS, out))
    assert plan['planned'] == 1
    return plan


# ---------------------------------------------------------------------------------------------------------------------------
# the probe: each form alone
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def probe_out(cuda_device):
    csrc = os.path.join(ROOT, 'learn_region_grow_amd', 'csrc')
    deps = [os.path.join(ROOT, 'tools', 'wave_tile_probe.hip'), os.path.join(csrc, 'lrg_async_units.inl')]
    if not os.path.exists(PROBE) or os.path.getmtime(PROBE) < max(os.path.getmtime(d) for d in deps):      # (built by __graft_entry__.build(); here for a tree that was not)
        os.makedirs(os.path.dirname(PROBE), exist_ok=True)
        subprocess.check_call(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-I', csrc, deps[0], '-o', PROBE],
                              stderr=subprocess.DEVNULL)
    r = subprocess.run([PROBE, 'units'], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode in (0, 1), r.stdout[-2000:] + r.stderr[-1000:]      # (1: values differ -- the tests below say which)
    return r.stdout


@pytest.mark.parametrize('form,rows', [(1, 'pooled rows'), (1, 'per-tile pool rows'), (2, 'pooled rows'), (3, 'pooled rows'), (3, 'per-tile pool rows')])
def test_every_sum_of_a_form_equals_the_host_chain(probe_out, form, rows):
    """96 slots x 8 rounds through a ring of 256 entries (three times round it), sixteen units: 2 heads x 96 slots x 256 sums, every slot with all its arrivals."""
    m = re.search(r'units form %d \([a-z -]+\), %s: sums (\d+) of (\d+) differ from the host chain; slots with all arrivals (\d+) of (\d+); abort word (\d+)' % (form, rows),
                  probe_out)
    assert m, probe_out
    bad, n, complete, slots, aborted = (int(v) for v in m.groups())
    assert (n, slots) == (2 * 96 * 256, 96)
    assert (bad, complete, aborted) == (0, 96, 0)


def test_probe_times_the_three_forms(probe_out):
    """(the figures themselves: profiles/unit_registers.txt)"""
    lat = re.findall(r'UNITS form (\d) \([a-z -]+\) latency: +(\d+) ticks', probe_out)
    cap = re.findall(r'UNITS form (\d) \([a-z -]+\) capacity: +(\d+) k tasks/s', probe_out)
    assert sorted(int(f) for f, _ in lat) == [1, 2, 3] and sorted(int(f) for f, _ in cap) == [1, 2, 3], probe_out
    assert all(int(v) > 0 for _, v in lat + cap)


# ---------------------------------------------------------------------------------------------------------------------------
# whole runs against the lock-step iterations
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def net(cuda_device):
    from learn_region_grow_amd.lrgnet import LrgNetHIP
    return LrgNetHIP(1, 1, 512, 512, 13, 0, device=cuda_device).load_weights(synthetic.make_synthetic_weights(**WEIGHT_KW))


def lock_step(net, rooms):
    from learn_region_grow_amd.grow import RegionGrower
    return RegionGrower(net, free_run=False, rooms_in_flight=4, rng='counter', seed=SEED, policy='net').run(rooms)


@pytest.fixture(scope='module')
def rooms_and_lock_step(net):
    """The six generator rooms of about 1.5 k points of tests/test_gpu_cu_roles.py, and what the lock-step iterations make of them (computed once)."""
    rooms = [small_room(700 + i, 1400 + 50 * i, room_id=20 + i) for i in range(6)]
    return rooms, lock_step(net, rooms)


def free_run(net, rooms, in_flight, **kw):
    from learn_region_grow_amd.grow import RegionGrower
    gr = RegionGrower(net, free_run=True, rooms_in_flight=in_flight, rng='counter', seed=SEED, policy='net', **kw)
    got = gr.run(rooms)
    assert gr.free_run and gr.S == in_flight
    return got


def same_as(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        same_regions(g.regions, w.regions)
        np.testing.assert_array_equal(g.cluster_label, w.cluster_label)
        np.testing.assert_array_equal(g.filled_label, w.filled_label)


@pytest.mark.parametrize('in_flight', [4, 26, 68, 100])
def test_free_running_labels_with_the_form_forced_on_equal_lock_step(net, rooms_and_lock_step, monkeypatch, in_flight):
    """(the switches are read on every call of the launch)"""
    rooms, want = rooms_and_lock_step
    monkeypatch.setenv(SWITCH, '1')
    got = free_run(net, rooms, in_flight)
    plan = last_plan()
    steps = sum(g.total_steps for g in got)
    print('%d slots, %s=1: %d regions, %d steps; plan %s' % (in_flight, SWITCH, sum(len(g.regions) for g in got), steps, plan))
    assert plan['gemv_units'] == 16 and plan['unit_regs'] == 1 and plan['n_slots'] == in_flight
    assert steps >= 100
    same_as(got, want)


def test_the_switch_unset_the_plan_takes_the_form_at_68_slots(net, rooms_and_lock_step, monkeypatch):
    rooms, want = rooms_and_lock_step
    monkeypatch.delenv(SWITCH, raising=False)
    got = free_run(net, rooms, 68)
    plan = last_plan()
    assert plan['gemv_units'] == 16 and plan['unit_regs'] == 1, plan
    same_as(got, want)


def test_the_switch_at_zero_keeps_the_teams(net, rooms_and_lock_step, monkeypatch):
    rooms, want = rooms_and_lock_step
    monkeypatch.setenv(SWITCH, '0')
    got = free_run(net, rooms, 68)
    plan = last_plan()
    assert plan['gemv_units'] == 16 and plan['unit_regs'] == 0, plan
    same_as(got, want)


def test_launches_of_one_and_a_half_milliseconds(net, rooms_and_lock_step, monkeypatch):
    """Every launch ends on its budget with evaluations in flight, which it finishes: the units leave when the fronts are done and start again with the next launch."""
    rooms, want = rooms_and_lock_step
    monkeypatch.setenv(SWITCH, '1')
    got = free_run(net, rooms, 68, free_run_budget_us=1500)
    assert last_plan()['unit_regs'] == 1
    same_as(got, want)


def test_rooms_that_run_out_in_the_middle_of_a_launch(net, rooms_and_lock_step, monkeypatch):
    """Two rooms on four slots and no time limit: two slots never have work, the other two finish inside the one launch -- the fronts are done while the engines wait."""
    rooms, want = rooms_and_lock_step
    monkeypatch.setenv(SWITCH, '1')
    got = free_run(net, rooms[:2], 4, free_run_budget_us=0)
    assert last_plan()['unit_regs'] == 1
    same_as(got, want[:2])


def test_two_runs_give_the_same_labels(net, rooms_and_lock_step, monkeypatch):
    rooms, _ = rooms_and_lock_step
    monkeypatch.setenv(SWITCH, '1')
    first, second = free_run(net, rooms, 26), free_run(net, rooms, 26)
    for a, b in zip(first, second):
        np.testing.assert_array_equal(a.cluster_label, b.cluster_label)
        np.testing.assert_array_equal(a.filled_label, b.filled_label)


def test_every_step_at_68_slots_logits_bit_for_bit(net, monkeypatch):
    """Three small rooms on 68 slots, one step per launch, every step audited (tests/step_audit.py): the logits are those of a dense evaluation of the same
    network, one instance at a time, bit for bit -- the pooled product's summation order is part of that."""
    from learn_region_grow_amd.grow import RegionGrower
    monkeypatch.setenv(SWITCH, '1')
    rooms = [small_room(520 + i, 900 + 400 * i, furniture=3, room_id=70 + i) for i in range(3)]
    runs = {}

    def oracle(seed):
        runs[seed] = [sa.oracle_run(r, seed, policy='net', net_fn=gpu_net_fn(net)) for r in rooms]
        return [w for w, _ in runs[seed]]
    seed, _ = seed_without_near_tie(oracle, range(123, 131), SAME_LOGITS_MARGIN)
    gr = RegionGrower(net, rooms_in_flight=68, rng='counter', seed=seed, policy='net', free_run=True)
    audit = sa.Audit(gr, rooms, runs[seed], 'free', logits=True)
    assert gr.free_run and gr.S == 68
    audit.run(lambda: gr.enqueue_free_run(steps=1, budget_us=0))      # (every step of the oracle's runs is met: Audit.run)
    assert last_plan()['unit_regs'] == 1 and audit.calls >= 20


def test_lite2_at_84_slots_keeps_the_four_teams(cuda_device, rooms_and_lock_step, monkeypatch):
    """512 pooled features: the form is for the paper's heads only, forced or not."""
    from learn_region_grow_amd.lrgnet import LrgNetHIP
    rooms, _ = rooms_and_lock_step
    monkeypatch.setenv(SWITCH, '1')
    lite2 = LrgNetHIP(1, 1, 512, 512, 13, 2, device=cuda_device).load_weights(synthetic.make_synthetic_weights(lite=2, **WEIGHT_KW))
    want = lock_step(lite2, rooms)
    got = free_run(lite2, rooms, 84)
    plan = last_plan()
    assert plan['gemv_units'] == 4 and plan['unit_regs'] == 0 and plan['unit_pairs'] == 0, plan
    same_as(got, want)
