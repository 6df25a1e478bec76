"""CPU: the host side of preprocess_gpu.preprocess_rooms -- the chunk plan, and the batched finish of eig='exact' on covariances from the
host version with a NumPy stand-in for the device solve (numpy.linalg.eigh, |w| descending, the PREP_EIG_SLACK flag rule restated)."""
import numpy as np
import pytest

from learn_region_grow_amd import preprocess, preprocess_gpu, synthetic


def _check_plan(sizes, budget):
    chunks = preprocess_gpu.plan_chunks(sizes, budget)
    assert [i for a, b in chunks for i in range(a, b)] == list(range(len(sizes)))        # order kept, every room exactly once
    for k, (a, b) in enumerate(chunks):
        assert b > a
        load = sum(sizes[a:b])
        assert load <= budget or b - a == 1                                               # within the budget, or one room alone
        if k + 1 < len(chunks):
            assert load + sizes[b] > budget                                               # (greedy: the next room did not fit)
    return chunks


def test_plan_chunks_at_every_room_boundary():
    sizes = [5, 3, 7, 2, 4]
    prefix = np.cumsum(sizes)
    for first in range(len(sizes)):
        for last in range(first, len(sizes)):
            load = sum(sizes[first:last + 1])
            for budget in (load - 1, load, load + 1):
                if budget >= 1:
                    _check_plan(sizes, budget)
    # a budget exactly at a boundary closes the chunk there; one below it, a room earlier
    assert preprocess_gpu.plan_chunks(sizes, int(prefix[1])) == [(0, 2), (2, 3), (3, 5)]
    assert preprocess_gpu.plan_chunks(sizes, int(prefix[1]) - 1) == [(0, 1), (1, 2), (2, 3), (3, 5)]
    assert preprocess_gpu.plan_chunks(sizes, int(prefix[-1])) == [(0, 5)]
    assert preprocess_gpu.plan_chunks(sizes, int(prefix[-1]) - 1) == [(0, 4), (4, 5)]


def test_plan_chunks_room_over_the_budget_and_single_room():
    assert preprocess_gpu.plan_chunks([4, 100, 4, 4], 10) == [(0, 1), (1, 2), (2, 4)]      # the large room is a chunk of its own
    assert preprocess_gpu.plan_chunks([100], 10) == [(0, 1)]
    assert preprocess_gpu.plan_chunks([7], 10) == [(0, 1)]
    assert preprocess_gpu.plan_chunks([], 10) == []
    assert preprocess_gpu.plan_chunks([3, 3, 3], 1) == [(0, 1), (1, 2), (2, 3)]
    with pytest.raises(ValueError):
        preprocess_gpu.plan_chunks([3], 0)


def _stand_in_device_solve(cov):
    """What lrg_preprocess eig_mode 2 hands the host, from another backward-stable solver: normals |V[smallest]|, un-normalised
    curvature, and the flags of csrc/lrg_preprocess.hip (prep_eig_point) restated."""
    w, V = np.linalg.eigh(cov)
    s = np.abs(w)
    idx = np.argsort(-s, axis=1, kind='stable')
    s = np.take_along_axis(s, idx, axis=1)
    v2 = np.abs(np.take_along_axis(V, idx[:, None, 2:3], axis=2)[:, :, 0])
    with np.errstate(invalid='ignore', divide='ignore'):
        cv = np.abs(s[:, 2] / (s[:, 0] + s[:, 1] + s[:, 2]))
        gap = s[:, 1] - s[:, 2]
        unsafe = ~(gap > 1e-6 * s[:, 0]) | np.isnan(cv)
        dv = preprocess_gpu.EXACT_SLACK * s[:, 0] / gap
        lo, hi = (v2 - dv[:, None]).astype(np.float32), (v2 + dv[:, None]).astype(np.float32)
        unsafe |= ((lo != hi) | (v2 < dv[:, None])).any(axis=1)
    return v2, cv, unsafe


def test_exact_finish_of_a_batch_equals_the_host_version():
    raws = [synthetic.generate_room_points(2500, seed, wlh=(1.6, 1.3, 1.0)).astype(np.float32) for seed in (1, 5, 7)]
    raws.append(synthetic.area5_shaped_room(3000, 79).astype(np.float32))
    want = [preprocess.preprocess_room(r[:, :6], r[:, 6].astype(int), r[:, 7].astype(int), return_cov=True) for r in raws]
    eq_start = np.concatenate(([0], np.cumsum([len(w['points']) for w in want])))
    cov = np.concatenate([w['cov'] for w in want]).reshape(-1, 3, 3)
    normals, curv, unsafe = _stand_in_device_solve(cov)
    feats = np.concatenate([w['points'] for w in want]).copy()
    feats[:, 9:12] = normals.astype(np.float32)
    for a, b in zip(eq_start[:-1], eq_start[1:]):
        feats[a:b, 12] = (curv[a:b] / curv[a:b].max()).astype(np.float32)
    fetched = []

    def fetch_cov(idx):
        fetched.append(len(idx))
        return cov[idx]
    got = preprocess_gpu.exact_finish_batch(eq_start, curv, feats, unsafe, fetch_cov, 13)
    assert len(fetched) <= 2                                       # one gather per pass, whatever the number of rooms
    assert len(got) == len(want)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g['points'], w['points'])
        np.testing.assert_array_equal(g['order'], w['order'])
        st = g['exact_stats']
        print('lapack share %.2f %% of %d points' % (100.0 * st['lapack_points'] / st['points'], st['points']))
        assert st['points'] == len(w['points'])
        assert st['lapack_points'] <= 0.15 * st['points'] + 8, st
