"""CPU: the host side of metrics_gpu -- the NumPy twin of the device pass (tests/metrics_twin.py) with metrics_gpu's own ground-truth
preparation and finish against sklearn and metrics.py, the refusal codes of lrg_metrics_batch through the loaded library (nothing is
launched for a refused call, so no device is needed), and the host range check of the labels."""
import ctypes

import numpy as np
import pytest

import metrics_twin
from learn_region_grow_amd import _lib, metrics, metrics_gpu

CASES = metrics_twin.cases()


@pytest.fixture(scope='module')
def host_results():
    return {name: (metrics.room_metrics(obj, lab), metrics.room_metrics_set_order(obj, lab)) for name, obj, lab in CASES}


@pytest.mark.parametrize('name,obj,lab', CASES, ids=[c[0] for c in CASES])
def test_twin_equals_host_and_sklearn(host_results, name, obj, lab):
    for order, want in zip(('size', 'set'), host_results[name]):
        got = metrics_twin.twin_room_metrics(obj, lab, order, with_scores=(order == 'size'))
        for key in ('prc', 'rcl', 'iou'):
            assert got[key] == want[key] or (np.isnan(got[key]) and np.isnan(want[key])), (order, key, got[key], want[key])
        np.testing.assert_array_equal(got['cluster_label2'], want['cluster_label2'])
        assert got['cluster_label2'].dtype == want['cluster_label2'].dtype
        if order == 'size':
            print('%s: |nmi - sklearn| %.2e  |ami - sklearn| %.2e' % (name, abs(got['nmi'] - want['nmi']), abs(got['ami'] - want['ami'])))
            assert got['ars'] == want['ars']
            assert abs(got['nmi'] - want['nmi']) <= 1e-12
            assert abs(got['ami'] - want['ami']) <= 1e-12
        else:
            assert set(got) == {'prc', 'rcl', 'iou', 'cluster_label2'}


def test_scores_special_cases_are_sklearns():
    assert metrics_gpu.scores_from_sums(100 * 100, 100 * 100, 100 * 100, 100, 1, 1, 0.0, 0.0, 0.0, 0.0) == dict(nmi=1.0, ami=1.0, ars=1.0)
    s = metrics_gpu.scores_from_sums(4 * 25 * 25, 100 * 100, 4 * 25 * 25, 100, 1, 4, 0.0, 1.3, 0.0, 0.0)
    assert s['nmi'] == 0.0 and s['ami'] == 0.0 and s['ars'] == 0.0
    # tp * tn past int64 at 100 k points: Python integers
    n = 100000
    s = metrics_gpu.scores_from_sums(n * n // 2 - 7, n * n // 2, n * n // 2, n, 2, 2, 0.69, 0.69, 0.6, 1e-5)
    assert 0.0 < s['ars'] < 1.0


def _i32(values):
    a = np.array(values, dtype=np.int32)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def test_workspace_and_refusals_without_a_device(hip_lib):
    E = _lib.LRG_EINVAL
    fake = ctypes.c_void_p(4096)                      # never dereferenced: every call below is refused before a launch
    keep = []

    def call(room_start, gt_start, n_cluster, n_rooms=None, ws=fake, ws_bytes=1 << 40, labels=fake):
        arrs = [_i32(room_start), _i32(gt_start), _i32(n_cluster)]
        keep.append(arrs)
        R = len(n_cluster) if n_rooms is None else n_rooms
        ps = [p for _, p in arrs]
        size = hip_lib.lrg_metrics_batch_workspace_bytes(ps[0], ps[1], ps[2], R)
        rc = hip_lib.lrg_metrics_batch(labels, fake, fake, fake, fake, ps[0], ps[1], ps[2], R, 0, ws, ws_bytes, fake, fake, fake, fake, fake,
                                       fake, None)
        return size, rc

    # the workspace of a good layout: every region of it, 256-byte aligned, and growing with the rooms
    good = ([0, 1000, 3000], [0, 5, 12], [7, 0])
    arrs = [_i32(v) for v in good]
    size2 = hip_lib.lrg_metrics_batch_workspace_bytes(arrs[0][1], arrs[1][1], arrs[2][1], 2)
    size1 = hip_lib.lrg_metrics_batch_workspace_bytes(arrs[0][1], arrs[1][1], arrs[2][1], 1)
    cells, cols, chunks = 5 * 8 + 7 * 1, 8 + 1, (5 * 8 + 5 * 1000 // 32 + 1) + (7 + 1 * 2000 // 32 + 1)
    floor = 4 * (2 * cells + 12 + 2 * cols) + 8 * (2000 + 1) + 8 * chunks
    assert size2 % 256 == 0 and size1 % 256 == 0 and 0 < size1 < size2
    assert floor <= size2 <= floor + 14 * 256 + 7 * 3 * 4 + 14 * 256
    assert call([1, 5], [0, 2], [1]) == (0, E - 90)                       # a start that does not begin at 0
    assert call([0, 5], [1, 2], [1]) == (0, E - 90)
    assert call([0, 5], [0, 2], [1], n_rooms=0) == (0, E - 90)
    assert call([0, 5, 3], [0, 2, 4], [1, 1]) == (0, E - 91)              # decreasing
    assert call([0, 5, 9], [0, 2, 1], [1, 1]) == (0, E - 91)
    assert call([0, 5, 5], [0, 2, 4], [1, 1]) == (0, E - 92)              # an empty room
    assert call([0, 5, 9], [0, 2, 2], [1, 1]) == (0, E - 92)              # a room without a GT row
    assert call([0, 5], [0, 2], [-1]) == (0, E - 93)
    assert call([0, 1 << 30], [0, 2], [1]) == (0, E - 94)                 # sum N past the numbering
    assert call([0, 5000], [0, 5000], [5000]) == (0, E - 94)              # 25 M cells in one room
    assert call([0, 1 << 29], [0, 1 << 12], [1 << 11]) == (0, E - 94)     # the chunk numbering: 2^12 2^29 / 32 >= 2^31
    size, rc = call(*good, labels=None)
    assert size == size2 and rc == E - 95
    assert call(*good, ws=None)[1] == E - 95
    assert call(*good, ws_bytes=size2 - 1)[1] == E - 96
    assert call(*good, ws=ctypes.c_void_p(4096 + 128))[1] == E - 96
    status = (ctypes.c_int32 * 2)()
    assert hip_lib.lrg_metrics_batch_status(None, arrs[0][1], arrs[1][1], arrs[2][1], 2, status, None) == E - 95
    assert hip_lib.lrg_metrics_batch_status(fake, arrs[0][1], arrs[1][1], arrs[2][1], 2, None, None) == E - 95
    assert hip_lib.lrg_metrics_batch_status(fake, arrs[0][1], arrs[1][1], arrs[2][1], 0, status, None) == E - 90


def test_host_labels_are_range_checked_before_any_device_work():
    obj = np.array([1, 1, 2, 2, 2])
    with pytest.raises(ValueError, match=r'outside \[0, C\]'):
        metrics_gpu.room_metrics_batch([obj], [np.array([1, 2, -1, 2, 1])])
    prep = [metrics_gpu.prepare_ground_truth(obj)]
    with pytest.raises(ValueError, match=r'outside \[0, C\]'):
        metrics_gpu.run_batch(prep, [np.array([1, 2, 3, 2, 1])], n_clusters=[2])
    with pytest.raises(ValueError):
        metrics_gpu.room_metrics_batch([obj], [np.array([1, 2, 1])])
    with pytest.raises(ValueError):
        metrics_gpu.prepare_ground_truth(obj, order='random')


def test_prepare_ground_truth_orders():
    obj = np.array([40, -7, 40, 3, 3, 40, 1000])
    size = metrics_gpu.prepare_ground_truth(obj, 'size')
    uniq, inv, count = np.unique(obj, return_inverse=True, return_counts=True)
    np.testing.assert_array_equal(size['gt_row'], inv)
    np.testing.assert_array_equal(size['order'], np.argsort(count)[::-1])
    np.testing.assert_array_equal(size['relabel'], [1, 2, 3, 4])
    assert size['unmatched_base'] == 1000 and size['n_gt'] == 4 and size['n'] == 7
    st = metrics_gpu.prepare_ground_truth(obj, 'set')
    np.testing.assert_array_equal(st['relabel'], [int(i) for i in set(obj)])
    np.testing.assert_array_equal(uniq[st['order']], st['relabel'])
