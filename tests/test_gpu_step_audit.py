"""GPU: every grow step of every formulation against the oracle's record of that step (step_audit.py), bit for bit.

Region records and labels say little about what a step PREPARES: under ground-truth masks the centre, the gathered rows and the
logits cannot change them at all, under the Bernoulli policy only through a flipped draw.  Here the growers are driven by hand,
one host call at a time, and after every call each ACTIVE slot's counts, box, mask, lists, centre, sample positions, packed rows,
flags and (Bernoulli policy) logits are read back and compared with grow_ref's hook record of that very step.

The rooms of median_rooms.py stop their regions at exactly the size boundaries of the medians, so the audit's centres reach every
form of csrc/lrg_median.h as dispatched by lrg_front_big_kernel (packed greedy), lrg_front_prepare (general front, the `wide` rooms),
lrg_front_all_medians (free-running launch) and lrg_median (nine-launch step) -- DESIGN.md section 3.1, `Which median serves which
size class`.  test_median_rooms_host.py states, without a GPU, that the rooms do so and that the comparer catches planted faults."""
import numpy as np
import pytest

import median_rooms as mr
import step_audit as sa
from conftest import seed_without_near_tie
from learn_region_grow_amd import synthetic
from test_gpu_grow import WEIGHT_KW, SAME_LOGITS_MARGIN, gpu_net_fn, small_room

pytestmark = pytest.mark.gpu
SEED = 5


def _net(cuda_device, ni=512, nn=512, F=13):
    from learn_region_grow_amd.lrgnet import LrgNetHIP
    return LrgNetHIP(1, 1, ni, nn, F, 0, device=cuda_device).load_weights(synthetic.make_synthetic_weights(feature_size=F, **WEIGHT_KW))


@pytest.fixture(scope='module')
def net(cuda_device):
    return _net(cuda_device)


@pytest.fixture(scope='module')
def net1024(cuda_device):
    return _net(cuda_device, 1024, 1024)


@pytest.fixture(scope='module')
def net12(cuda_device):
    return _net(cuda_device, F=12)


class Oracles:
    """Oracle runs under ground-truth masks, made on first use and shared by all forms (the big room's takes ~15 s of CPU)."""

    def __init__(self):
        self.made = {}

    def get(self, name, **kw):
        key = (name,) + tuple(sorted(kw.items()))
        if key not in self.made:
            okw = {k: kw.pop(k) for k in ('Ni', 'Nn', 'restarts') if k in kw}
            room = getattr(mr, name)(**kw)
            self.made[key] = (room,) + sa.oracle_run(room, SEED, **okw)
        room, want, recs = self.made[key]
        return room, (want, recs)


@pytest.fixture(scope='module')
def oracles():
    return Oracles()


def _grower(net, n_rooms=1, policy='gt', seed=SEED, **kw):
    from learn_region_grow_amd.grow import RegionGrower
    return RegionGrower(net, rooms_in_flight=n_rooms, rng='counter', seed=seed, policy=policy, **kw)


def _free_call(gr):
    return lambda: gr.enqueue_free_run(steps=1, budget_us=0)


# ---------------------------------------------------------------------------------------------------------------------------
# ground-truth masks: the rooms of the size boundaries
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['greedy', 'greedy_row_major', 'wide', 'free'])
def test_classes_room(net, oracles, monkeypatch, case):
    """Regions of exactly 256 / 257 / 1024 / 1025 / 4096 / 4097 / 16384 / 16385 points, 500 steps, every one audited.  greedy: lrg_front_big_kernel up
    to the sampled selection (48 keys per thread, bracket path and full bisection); greedy_row_major: the same from the [n, F] rows (LRG_NO_CHAN_MAJOR=1);
    wide: lrg_front_kernel<7>, whose lrg_front_prepare takes wave_r<4> / <16> / wave_r64 / block_regs<16> / <48>; free: lrg_front_all_medians with
    both radix groupings and the bisection over the list above 16 Ki."""
    room, oracle = oracles.get('classes_room', wide=True) if case == 'wide' else oracles.get('classes_room')
    if case == 'greedy_row_major':
        monkeypatch.setenv('LRG_NO_CHAN_MAJOR', '1')
    form = {'wide': 'general', 'free': 'free'}.get(case, 'greedy')
    gr = _grower(net, free_run=form == 'free')
    audit = sa.Audit(gr, [room], [oracle], form)
    assert gr.have_pvox == (case != 'wide') and (gr.d_chan is None) == (case == 'greedy_row_major')
    audit.run(_free_call(gr) if form == 'free' else gr.enqueue_iteration)
    assert audit.calls >= 500


@pytest.mark.parametrize('case', ['step', 'restart_group', 'graph', 'sets_of_1024'])
def test_cut_room(net, net1024, oracles, case):
    """The six smallest strips (regions up to 4097 points).  step: the nine-launch lrg_grow_step with its padded sets and per-sample flags
    (lrg_median, lrg_prepare); restart_group: two restarts in groups of two slots (lrg_front_kernel<1> / lrg_advance / <4>); graph: four packed
    iterations per HIP-graph replay, audited after every replay; sets_of_1024: 1024 + 1024 points per set, lrg_front_kernel<7> by set size."""
    import torch
    okw, gkw, form, every, nt = {}, {}, 'greedy', True, net
    if case == 'step':
        gkw, form = dict(packed=False), 'step'
    elif case == 'restart_group':
        okw, gkw, form = dict(restarts=2), dict(restarts=2, group_size=2, packed=True), 'general'
    elif case == 'graph':
        gkw, every = dict(packed=True, free_run=False, graph_iterations=4), False
    elif case == 'sets_of_1024':
        okw, gkw, form, nt = dict(Ni=1024, Nn=1024), dict(packed=True), 'general', net1024
    room, oracle = oracles.get('cut_room', **okw)
    with torch.cuda.stream(torch.cuda.Stream()):          # (a HIP graph is not captured on the null stream)
        gr = _grower(nt, **gkw)
        audit = sa.Audit(gr, [room], [oracle], form, every_record=every)
        audit.run(gr.enqueue_graph if case == 'graph' else gr.enqueue_iteration)
        torch.cuda.synchronize()
    if case == 'graph':
        # a replay is four steps, and it leaves its slot ACTIVE unless its last iteration ended a region for want of neighbours (the box
        # query stops the slot; the next iteration commits it) or ended the room: at most once per region, and once more
        assert gr._graph is not None and 4 * audit.calls >= len(oracle[1])
        assert len(audit.seen[0]) >= audit.calls - len(oracle[0].regions) - 1


@pytest.mark.parametrize('case', ['greedy', 'wide'])
def test_big_room(net, oracles, case):
    """Regions of exactly 49152 and 49153 points: the last size of the sampled selection / of block_regs<48>, and the first of the bisection over the
    list in memory (lrg_select2), in lrg_front_big_kernel (greedy) and in lrg_front_prepare (wide)."""
    room, oracle = oracles.get('big_room', wide=case == 'wide')
    gr = _grower(net, free_run=False)
    audit = sa.Audit(gr, [room], [oracle], 'general' if case == 'wide' else 'greedy')
    audit.run(gr.enqueue_iteration)
    assert audit.calls >= 516


@pytest.mark.parametrize('case', ['greedy', 'wide', 'free'])
def test_even_room(net, oracles, case):
    """Over ninety even counts between 16 Ki and 49664, three of them above 49152: the MEAN of the two middle keys -- lrg_select2 asked for two ranks -- in
    lrg_front_big_kernel (greedy), lrg_front_prepare (wide) and, from 16 Ki on, lrg_front_all_medians (free); below 49152 the sampled selection and
    block_regs<48> on even counts."""
    room, oracle = oracles.get('even_room', wide=case == 'wide')
    form = {'wide': 'general', 'free': 'free'}.get(case, 'greedy')
    gr = _grower(net, free_run=form == 'free')
    audit = sa.Audit(gr, [room], [oracle], form)
    audit.run(_free_call(gr) if form == 'free' else gr.enqueue_iteration)
    assert audit.calls >= 258


# ---------------------------------------------------------------------------------------------------------------------------
# the Bernoulli policy on small rooms, several in flight: the full audit, logits included
# ---------------------------------------------------------------------------------------------------------------------------
def _small_rooms(case, F=13):
    rooms = [small_room(520 + i, 900 + 400 * i, furniture=3, room_id=70 + i) for i in range(3)]
    if case == 'general':
        # one lone point 2100 voxels away in y: the room -- and with it the set -- has no packed voxel words (lrg_front_kernel<7>)
        r = rooms[0]
        far = r['points'][:1].copy()
        far[0, 1] += np.float32(210.0)
        rooms[0] = dict(points=np.concatenate([r['points'], far]), obj_id=np.concatenate([r['obj_id'], [int(r['obj_id'].max()) + 1]]),
                        order=np.concatenate([r['order'], [len(r['order'])]]), room_id=r['room_id'])
    return [dict(r, points=np.ascontiguousarray(r['points'][:, :F])) for r in rooms]


NET_CASES = {'greedy': dict(free_run=False), 'general': dict(free_run=False), 'restart_group': dict(restarts=2, group_size=2, packed=True),
             'free': dict(free_run=True), 'F12': dict(free_run=False)}
NET_FORMS = {'greedy': 'greedy', 'general': 'general', 'restart_group': 'general', 'free': 'free', 'F12': 'greedy'}


@pytest.fixture(scope='module')
def net_oracles():
    return {}


@pytest.mark.parametrize('case', list(NET_CASES))
def test_small_rooms_under_the_bernoulli_policy(net, net12, net_oracles, case):
    """Three rooms in flight (six slots with restart groups), so that the packed rows of different slots share tiles.  The oracle evaluates the
    same GPU network one instance at a time (dense sets); include/lrg_hip.h promises the packed evaluation the same bits, and the logits are
    compared as such."""
    nt = net12 if case == 'F12' else net
    rooms = _small_rooms(case, 12 if case == 'F12' else 13)
    restarts = NET_CASES[case].get('restarts', 0)
    okey = (case if case in ('general', 'F12') else 'base', restarts)
    if okey not in net_oracles:
        runs = {}

        def oracle(seed):
            runs[seed] = [sa.oracle_run(r, seed, policy='net', net_fn=gpu_net_fn(nt), restarts=restarts) for r in rooms]
            return [w for w, _ in runs[seed]]
        seed, _ = seed_without_near_tie(oracle, range(123, 131), SAME_LOGITS_MARGIN)
        net_oracles[okey] = (seed, runs[seed])
    seed, oracle_runs = net_oracles[okey]
    gr = _grower(nt, n_rooms=len(rooms), policy='net', seed=seed, **NET_CASES[case])
    form = NET_FORMS[case]
    audit = sa.Audit(gr, rooms, oracle_runs, form, logits=True)
    assert gr.S == len(rooms) * (2 if case == 'restart_group' else 1)
    audit.run(_free_call(gr) if form == 'free' else gr.enqueue_iteration)


def test_lite2_pooled_product_units_at_84_slots_under_the_bernoulli_policy(cuda_device):
    """Lite 2 (convolutions 64, 64, 256: 512 pooled features, four pooled-product units) with 84 slots in flight, three of them on rooms: the first slot
    count at which the launch plan used to hand the units' tasks to half-teams written for 1024 pooled features (csrc/lrg_async_plan.inl, plan_units; the
    plans: tests/test_async_plan.py).  Every step's logits are those of a dense evaluation of the same lite-2 network, one instance at a time, bit for
    bit -- from the first step on, without waiting for a draw to flip.  The regions and labels of whole runs at 84 and 148 slots:
    tests/test_gpu_free_run_shapes.py."""
    from learn_region_grow_amd.lrgnet import LrgNetHIP
    nt = LrgNetHIP(1, 1, 512, 512, 13, 2, device=cuda_device).load_weights(synthetic.make_synthetic_weights(lite=2, **WEIGHT_KW))
    rooms = _small_rooms('free')
    runs = {}

    def oracle(seed):
        runs[seed] = [sa.oracle_run(r, seed, policy='net', net_fn=gpu_net_fn(nt)) for r in rooms]
        return [w for w, _ in runs[seed]]
    seed, _ = seed_without_near_tie(oracle, range(123, 131), SAME_LOGITS_MARGIN)
    gr = _grower(nt, n_rooms=84, policy='net', seed=seed, free_run=True)
    audit = sa.Audit(gr, rooms, runs[seed], 'free', logits=True)
    assert gr.free_run and gr.S == 84
    audit.run(_free_call(gr))      # (every step of the oracle's runs is met: Audit.run)
