"""GPU: free-running launches (lrg_grow_async) on the supported networks that are NOT the paper's -- lite 2 at the slot counts of the pooled-product units, and
the paper's convolutions under narrower heads -- against the lock-step iterations, which promise the same bits (include/lrg_hip.h): regions and labels exactly.

Two pieces of the launch are written for the paper's shape only, and the launch plan (csrc/lrg_async_plan.inl) grants them to that shape only:
  lrg_async_gemv_unit2       half-teams in the pooled-product units: two loads of 512 floats per slot, 1024 pooled features.  Lite 2 has 512 (convolutions 64, 64,
                             256) and four units; from 84 slots in flight, where the half-teams switch on for the paper's network, it keeps the four-wavefront units.
  lrg_team_head_tile_reg     the head tiles of a register-tile launch, the default from 1 to 176 slots: heads 64 -> 256 -> 128 -> 2.  Another head stack on the paper's
                             convolutions (the C API accepts them: packed_shapes, csrc/lrg_net.hip) takes the one-kernel launch, whose team tiles are general.
The plans themselves, without a GPU: tests/test_async_plan.py (the rows lite2/, h128/, h256x64/ of tests/golden/async_plan_table.txt).  Lite 2's units at 84 slots
step by step, logits bit for bit against dense evaluations: tests/test_gpu_step_audit.py.  The lock-step side at lite 2 is tied to the oracle by
tests/test_gpu_grow.py::test_feature_size_and_lite_variants; the narrow-head networks are anchored here, by a float64 forward pass."""
import numpy as np
import pytest

from learn_region_grow_amd import synthetic
from oracle import lrgnet_ref
from test_gpu_grow import WEIGHT_KW, small_room, same_regions
from test_gpu_net import close

pytestmark = pytest.mark.gpu
SEED = 31
HEADS = {'h128': [128, 64], 'h256x64': [256, 64]}      # (the labels of the plan table; the second differs from the paper's 256, 128 in the second width only)


@pytest.fixture(scope='module')
def rooms():
    """Six generator rooms of about 1.5 k points (those of test_gpu_branch_tile_pairs.py)."""
    return [small_room(700 + i, 1400 + 50 * i, room_id=20 + i) for i in range(6)]


def _lock_step(net, rooms):
    """What the lock-step iterations make of the rooms (the slot count does not enter: the draws are per room)."""
    from learn_region_grow_amd.grow import RegionGrower
    return RegionGrower(net, free_run=False, rooms_in_flight=4, rng='counter', seed=SEED, policy='net').run(rooms)


def _free_run_equals(net, rooms, want, in_flight, waves=0):
    from learn_region_grow_amd.grow import RegionGrower
    gr = RegionGrower(net, free_run=True, free_run_waves=waves, rooms_in_flight=in_flight, rng='counter', seed=SEED, policy='net')
    got = gr.run(rooms)
    assert gr.free_run and gr.S == in_flight
    steps = sum(g.total_steps for g in got)
    print('%d slots: %d rooms, %d regions, %d steps' % (in_flight, len(got), sum(len(g.regions) for g in got), steps))
    assert steps >= 100
    assert len(got) == len(want)
    for g, w in zip(got, want):
        same_regions(g.regions, w.regions)
        np.testing.assert_array_equal(g.cluster_label, w.cluster_label)
        np.testing.assert_array_equal(g.filled_label, w.filled_label)


# ---------------------------------------------------------------------------------------------------------------------------
# lite 2: 512 pooled features
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lite2(cuda_device, rooms):
    from learn_region_grow_amd.lrgnet import LrgNetHIP
    net = LrgNetHIP(1, 1, 512, 512, 13, 2, device=cuda_device).load_weights(synthetic.make_synthetic_weights(lite=2, **WEIGHT_KW))
    return net, _lock_step(net, rooms)


@pytest.mark.parametrize('in_flight', [84, 148])
def test_lite2_with_the_units_slot_counts(lite2, rooms, in_flight):
    """84: the first slot count that took half-teams; 148: the last with units in the one-kernel launch."""
    net, want = lite2
    _free_run_equals(net, rooms, want, in_flight)


# ---------------------------------------------------------------------------------------------------------------------------
# the paper's convolutions, other heads
# ---------------------------------------------------------------------------------------------------------------------------
def _heads_net(cuda_device, heads):
    from learn_region_grow_amd.lrgnet import LrgNetHIP
    w = synthetic.make_synthetic_weights(head_channels=heads, **WEIGHT_KW)
    net = LrgNetHIP(1, 1, 512, 512, 13, 0, device=cuda_device)
    net.conv2_channels = list(heads)      # (variable_shapes and the weights struct follow it)
    return net.load_weights(w), w


@pytest.fixture(scope='module')
def heads_nets(cuda_device):
    made = {}

    def get(name, rooms=None):
        if name not in made:
            made[name] = list(_heads_net(cuda_device, HEADS[name])) + [None]
        if rooms is not None and made[name][2] is None:
            made[name][2] = _lock_step(made[name][0], rooms)
        return made[name]
    return get


@pytest.mark.parametrize('name', sorted(HEADS))
def test_narrow_heads_forward_packed_against_float64(cuda_device, heads_nets, name):
    """The anchor of the two tests below: lrg_forward_packed (what a lock-step iteration evaluates) on this network against the oracle's forward pass in
    float64 with the same widths, to the project's tolerance (test_gpu_net.close: 1e-4 + 1e-5 |x|).  Ragged row counts: 1, 31, 33 (a tile less one, a tile
    and one), 512 (a full set), a whole tile and a few rows, on either side."""
    import torch
    net, w, _ = heads_nets(name)
    assert [int(net._w.head_ch[i]) for i in range(net._w.n_head)] == HEADS[name] + [2]
    rows_in = np.array([1, 31, 33, 512, 64, 7], dtype=np.int32)
    rows_nb = np.array([33, 1, 512, 31, 5, 96], dtype=np.int32)
    B, F, cap = len(rows_in), 13, 1024
    rs = np.random.RandomState(7)
    xi = [(rs.randn(1, n, F) * 0.5).astype(np.float32) for n in rows_in]
    xn = [(rs.randn(1, n, F) * 0.5).astype(np.float32) for n in rows_nb]
    pin, pnb = np.full((cap, F), np.nan, np.float32), np.full((cap, F), np.nan, np.float32)      # (whatever lies past the counts must not matter)
    rin, rnb = np.full(cap, -7, np.int32), np.full(cap, -7, np.int32)
    off_in, off_nb = np.concatenate([[0], np.cumsum(rows_in)]), np.concatenate([[0], np.cumsum(rows_nb)])
    assert off_in[-1] <= cap and off_nb[-1] <= cap
    for b in range(B):
        pin[off_in[b]:off_in[b + 1]] = xi[b][0]; rin[off_in[b]:off_in[b + 1]] = b
        pnb[off_nb[b]:off_nb[b + 1]] = xn[b][0]; rnb[off_nb[b]:off_nb[b + 1]] = b
    t = lambda a: torch.from_numpy(a).to(cuda_device)
    add, rmv, pooled = net.forward_packed(t(pin), t(pnb), t(rin), t(rnb), t(np.array([off_in[-1], off_nb[-1]], np.int32)), B)
    torch.cuda.synchronize()
    add, rmv, pooled = add.cpu().numpy(), rmv.cpu().numpy(), pooled.cpu().numpy()
    assert pooled.shape == (B, 1024)
    for b in range(B):
        wadd, wrmv, acts = lrgnet_ref.forward(w, xi[b], xn[b], dtype=np.float64, return_acts=True, head_channels=HEADS[name])
        assert [h.shape[-1] for h in acts['add_hidden']] == HEADS[name]
        close(pooled[b], acts['pooled'][0], 'pooled, instance %d' % b)
        close(add[off_nb[b]:off_nb[b + 1]], wadd[0], 'add, instance %d' % b)
        close(rmv[off_in[b]:off_in[b + 1]], wrmv[0], 'rmv, instance %d' % b)


@pytest.mark.parametrize('name,in_flight,waves', [('h128', 4, 0), ('h128', 68, 0), ('h128', 68, 1), ('h256x64', 68, 0)])
def test_narrow_heads_free_running_equals_lock_step(heads_nets, rooms, name, in_flight, waves):
    """4 and 68 slots: on the paper's network the two-part and the one-part register tiles; here the one-kernel launch with eight (heads 128) or sixteen
    (heads 256) pooled-product units and general team head tiles -- also where register tiles are asked for by name (waves = 1)."""
    net, _, want = heads_nets(name, rooms)
    _free_run_equals(net, rooms, want, in_flight, waves)
