"""GPU: metrics_gpu.room_metrics_batch (lrg_metrics_batch) against metrics.py and sklearn on the labelings of tests/metrics_twin.py:
single classes / clusters, a perfect labeling, a live lower bound of the nij range, gapped and negative ids, tables on both sides of
the LDS budget (metrics_twin.LDS_CELLS = 8192 cells: 64 x 128 is the last table counted in LDS, 64 x 129 and 3 x 5001 take global
atomics), a size that is no multiple of 64, N = 1, N = 2 and the six golden rooms.

nmi / ami tolerance 1e-9 absolute: at N <= 6000 the lgamma table's values are below 5e4, where a float64 ulp is 7e-12; nine table
terms of a device lgamma a few ulp from libm's move a term of the EMI sum by a relative ~1e-10, and the AMI denominators of these
inputs are no smaller than ~0.1."""
import numpy as np
import pytest
import torch

import metrics_twin
from learn_region_grow_amd import _lib, metrics, metrics_gpu

pytestmark = pytest.mark.gpu
CASES = metrics_twin.cases()
GOLDEN_NAMES = [c[0] for c in metrics_twin.golden_rooms()]
RAW_KEYS = ('cluster_label2', 'best_iou', 'dt_match', 'gt_match', 'int_sums', 'float_sums', 'status')


@pytest.fixture(scope='module')
def host():
    """The references, computed once: metrics.room_metrics (with sklearn's scores) and metrics.room_metrics_set_order."""
    return {name: dict(size=metrics.room_metrics(obj, lab), set=metrics.room_metrics_set_order(obj, lab, with_sklearn=False))
            for name, obj, lab in CASES}


@pytest.fixture(scope='module')
def batch(cuda_device):
    """All cases as one batch, in both orders, and the raw device outputs of the 'size' batch."""
    objs, labs = [c[1] for c in CASES], [c[2] for c in CASES]
    prep = [metrics_gpu.prepare_ground_truth(o, 'size') for o in objs]
    return dict(size=metrics_gpu.room_metrics_batch(objs, labs, order='size', device=cuda_device),
                set=metrics_gpu.room_metrics_batch(objs, labs, order='set', device=cuda_device),
                prep=prep, raw=metrics_gpu.run_batch(prep, labs, device=cuda_device))


def _same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


@pytest.mark.parametrize('k', range(len(CASES)), ids=[c[0] for c in CASES])
def test_matching_outputs_equal_the_host(host, batch, k):
    name = CASES[k][0]
    for order in ('size', 'set'):
        got, want = batch[order][k], host[name][order]
        for key in ('prc', 'rcl', 'iou'):
            assert _same(got[key], want[key]), (order, key, got[key], want[key])
        np.testing.assert_array_equal(got['cluster_label2'], want['cluster_label2'])


@pytest.mark.parametrize('k', range(len(CASES)), ids=[c[0] for c in CASES])
def test_scores_against_sklearn(host, batch, k):
    name = CASES[k][0]
    for order in ('size', 'set'):
        got, want = batch[order][k], host[name]['size']
        print('%s %s: |nmi - sklearn| %.3e  |ami - sklearn| %.3e' % (name, order, abs(got['nmi'] - want['nmi']), abs(got['ami'] - want['ami'])))
        assert got['ars'] == want['ars']
        assert abs(got['nmi'] - want['nmi']) <= 1e-9
        assert abs(got['ami'] - want['ami']) <= 1e-9


def test_room_lines_of_the_golden_rooms(host, batch):
    for k, (name, obj, lab) in enumerate(CASES):
        if name not in GOLDEN_NAMES:
            continue
        want = metrics.room_line(5, k, host[name]['size'])
        assert metrics.room_line(5, k, batch['size'][k]) == want
        set_want = dict(host[name]['set'], **{s: host[name]['size'][s] for s in ('nmi', 'ami', 'ars')})
        assert metrics.room_line(5, k, batch['set'][k]) == metrics.room_line(5, k, set_want)


def test_batch_equals_every_room_alone_and_repeats(cuda_device, batch):
    raw = batch['raw']
    again = metrics_gpu.run_batch(batch['prep'], [c[2] for c in CASES], device=cuda_device)
    for key in RAW_KEYS:
        assert raw[key].tobytes() == again[key].tobytes(), key
    assert not raw['status'].any()
    for k, (name, obj, lab) in enumerate(CASES):
        one = metrics_gpu.run_batch([batch['prep'][k]], [lab], device=cuda_device)
        s0, s1 = raw['room_start'][k], raw['room_start'][k + 1]
        g0, g1 = raw['gt_start'][k], raw['gt_start'][k + 1]
        c0, c1 = raw['cluster_start'][k], raw['cluster_start'][k + 1]
        assert one['cluster_label2'].tobytes() == raw['cluster_label2'][s0:s1].tobytes(), name
        assert one['best_iou'].tobytes() == raw['best_iou'][g0:g1].tobytes(), name
        assert one['dt_match'].tobytes() == raw['dt_match'][c0:c1].tobytes(), name
        for key in ('gt_match', 'int_sums', 'float_sums', 'status'):
            assert one[key][0].tobytes() == raw[key][k].tobytes(), (name, key)


def test_device_tensors_give_the_same_result(cuda_device, batch):
    pick = [2, 5, 9, len(CASES) - 3]
    objs, labs = [CASES[k][1] for k in pick], [CASES[k][2] for k in pick]
    dev_labs = [torch.from_numpy(np.asarray(lab)).to(cuda_device) for lab in labs]
    got = metrics_gpu.room_metrics_batch(objs, dev_labs, device=cuda_device)
    mixed = metrics_gpu.room_metrics_batch(objs, [dev_labs[0], labs[1], dev_labs[2], labs[3]], device=cuda_device)
    for k, g, m in zip(pick, got, mixed):
        want = batch['size'][k]
        for res in (g, m):
            for key in ('prc', 'rcl', 'iou', 'nmi', 'ami', 'ars'):
                assert _same(res[key], want[key]), key
            np.testing.assert_array_equal(res['cluster_label2'], want['cluster_label2'])


def test_without_scores(cuda_device, batch):
    got = metrics_gpu.room_metrics_batch([c[1] for c in CASES], [c[2] for c in CASES], with_scores=False, device=cuda_device)
    for g, want in zip(got, batch['size']):
        assert set(g) == {'prc', 'rcl', 'iou', 'cluster_label2'}
        for key in ('prc', 'rcl', 'iou'):
            assert _same(g[key], want[key])
        np.testing.assert_array_equal(g['cluster_label2'], want['cluster_label2'])


def test_out_of_range_device_label_flags_its_room_only(cuda_device, batch):
    """The library's guard: the bad point is skipped, the room's status word is raised, the other rooms keep their bits."""
    pick = [3, 5, 6, 9]                          # an LDS table, the bad room (LDS), a global-atomics table, an LDS table
    prep = [batch['prep'][k] for k in pick]
    labs = [torch.from_numpy(np.asarray(CASES[k][2])).to(cuda_device) for k in pick]
    good = metrics_gpu.run_batch(prep, labs, device=cuda_device)
    for bad_value, n_clusters in ((-3, None), (10, [int(CASES[k][2].max()) for k in pick])):
        bad = [lab.clone() for lab in labs]
        bad[1][17] = bad_value
        raw = metrics_gpu.run_batch(prep, bad, device=cuda_device, n_clusters=n_clusters)
        assert raw['status'].tolist() == [0, 1, 0, 0]
        assert raw['int_sums'][1][3] == len(CASES[pick[1]][1]) - 1          # the point was left out
        for r in (0, 2, 3):
            s0, s1 = raw['room_start'][r], raw['room_start'][r + 1]
            g0, g1 = raw['gt_start'][r], raw['gt_start'][r + 1]
            assert raw['cluster_label2'][s0:s1].tobytes() == good['cluster_label2'][s0:s1].tobytes()
            assert raw['best_iou'][g0:g1].tobytes() == good['best_iou'][g0:g1].tobytes()
            for key in ('gt_match', 'int_sums', 'float_sums'):
                assert raw[key][r].tobytes() == good[key][r].tobytes()
    with pytest.raises(_lib.LrgHipError, match='room 1'):
        bad = [lab.clone() for lab in labs]
        bad[1][17] = -3
        metrics_gpu.room_metrics_batch([CASES[k][1] for k in pick], bad, device=cuda_device)
