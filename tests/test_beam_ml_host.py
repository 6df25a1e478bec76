"""CPU: the beam search's test twin (tests/beam_ml_ref.py) -- equal to oracle/beam_ref.py under 'np', its 'ml' terms equal to a
literal restatement of the reference's per-child loops, its follow mode accepting its own trace and rejecting a refutable one --
and the command line's acceptance of ``--beam B --scoring ml``."""
import copy

import numpy as np
import pytest

import beam_ml_ref
from beam_ml_ref import small_room
from learn_region_grow_amd import synthetic
from oracle import beam_ref, rng_ref


@pytest.fixture(scope='module')
def weights():
    return synthetic.make_synthetic_weights(seed=0)


@pytest.fixture(scope='module')
def furniture_room():
    return small_room(710, 1200, furniture=3)


@pytest.fixture(scope='module')
def ml_free_run(weights, furniture_room):
    """The twin's own 'ml' run of the furniture room (BW = SW = 2), computed once and left unchanged"""
    room = furniture_room
    return beam_ml_ref.beam_room(room['points'], room['obj_id'], room['order'], weights, rng_ref.CounterStream(41, 0), beam_width=2,
                                 search_width=2, scoring='ml')


def _same(got, want):
    assert got.total_steps == want.total_steps
    assert len(got.regions) == len(want.regions)
    for g, w in zip(got.regions, want.regions):
        assert set(g) == set(w)
        for k in w:
            assert g[k] == w[k] or (isinstance(w[k], float) and np.isnan(w[k]) and np.isnan(g[k])), (k, g, w)
    np.testing.assert_array_equal(got.cluster_label, want.cluster_label)
    np.testing.assert_array_equal(got.filled_label, want.filled_label)


@pytest.mark.parametrize('policy', ['net', 'gt'])
@pytest.mark.parametrize('which', ['furniture', 'plain'])
def test_np_twin_equals_the_oracle(weights, furniture_room, which, policy):
    room = furniture_room if which == 'furniture' else small_room(700, 600)
    kw = dict(beam_width=2, search_width=2, policy=policy)
    want = beam_ref.beam_room(room['points'], room['obj_id'], room['order'], weights, rng_ref.CounterStream(41, 0), **kw)
    got = beam_ml_ref.beam_room(room['points'], room['obj_id'], room['order'], weights, rng_ref.CounterStream(41, 0), scoring='np', **kw)
    _same(got, want)
    assert all(score == size for _, _, entries in got.beam_trace for _, size, score in entries)


def _literal_sides(neighbor_points, inlier_points, add_conf, rmv_conf, add_mask, rmv_mask, center, resolution, num_neighbor):
    """test_beam_search.py:234-257 row by row with Python sets of voxel tuples; float32 confidence, log and division, the terms of a
    side summed in float64 (the widths the project fixed, oracle/grow_ref.py:161-170).  -> (add terms, rmv terms, addLogProb, rmvLogProb)"""
    neighbor_points = np.array(neighbor_points, dtype=np.float32)[None]
    inlier_points = np.array(inlier_points, dtype=np.float32)[None]
    res32, n32 = np.float32(resolution), np.float32(num_neighbor)
    out = []
    with np.errstate(divide='ignore'):
        for pts, conf, mask in ((neighbor_points, add_conf, add_mask), (inlier_points, rmv_conf, rmv_mask)):
            sel = pts[0, :, :][mask]
            sel[:, :2] += center[:2]
            voxels = np.round(sel[:, :3] / res32).astype(int)
            vset = set([tuple(p) for p in voxels])
            terms, total = [], 0.0
            for i in range(len(pts[0])):
                pts[0, i, :2] += center[:2]
                p = tuple(np.round(pts[0, i, :3] / res32).astype(int))
                if p in vset:
                    t = np.log(np.float32(conf[i])) / n32
                else:
                    t = np.log(np.float32(1) - np.float32(conf[i])) / n32
                assert t.dtype == np.float32
                terms.append(t)
                total += float(t)
            out.append((np.array(terms, dtype=np.float32), total))
    return out[0][0], out[1][0], out[0][1], out[1][1]


@pytest.mark.parametrize('seed', range(6))
def test_ml_terms_equal_the_literal_restatement(seed):
    """N = 8 rows; voxels shared between rows (a copy of a fired row counts as fired), a padded set (rows 5.. are copies of 0..4), a
    confidence of exactly 0 and of exactly 1 (log 0 = -inf is a legal term)."""
    rs = np.random.RandomState(seed)
    N, F, res = 8, 13, 0.1
    center = (rs.randn(F) * 0.3).astype(np.float32)

    def rows():
        r = (rs.randn(N, F) * 0.25).astype(np.float32)
        r[3, :3] = r[1, :3]                                   # two rows, one voxel
        src = rs.randint(0, 5, size=N - 5)
        r[5:] = r[src]                                        # the padded set: copies
        return r, src
    neighbor, src_n = rows()
    inlier, src_i = rows()

    def confs(src):
        c = rs.uniform(0.02, 0.98, size=N).astype(np.float32)
        c[5:] = c[src]
        return c
    add_conf, rmv_conf = confs(src_n), confs(src_i)
    add_conf[0], rmv_conf[2] = 0.0, 1.0
    add_mask = rs.uniform(size=N) < 0.4
    rmv_mask = rs.uniform(size=N) < 0.4
    add_mask[1], add_mask[3] = True, False                    # of the two rows in one voxel, one draw fires
    want = _literal_sides(neighbor, inlier, add_conf, rmv_conf, add_mask, rmv_mask, center, res, N)
    got = beam_ml_ref.child_sides(neighbor, inlier, add_conf, rmv_conf, add_mask, rmv_mask, center, res, N)
    np.testing.assert_array_equal(got['add_terms'], want[0])
    np.testing.assert_array_equal(got['rmv_terms'], want[1])
    for g, w in ((got['add'], want[2]), (got['rmv'], want[3])):
        assert g == w or abs(g - w) <= 8 * 2.0 ** -52 * abs(w)      # (NumPy's pairwise float64 sum against the sequential one)
    assert got['add_terms'][3] == np.log(add_conf[3]) / np.float32(N)      # row 3 did not fire, its voxel did
    s, e = beam_ml_ref.child_score(-1.25, 1e-9, got)
    assert s == (-1.25 + got['add']) + got['rmv'] and e >= 1e-9
    assert beam_ml_ref.child_score(0.0, 0.0, dict(got, add=-np.inf))[0] == -np.inf


def test_ml_differs_from_np_and_carries_bounds(weights, furniture_room, ml_free_run):
    room = furniture_room
    base = beam_ref.beam_room(room['points'], room['obj_id'], room['order'], weights, rng_ref.CounterStream(41, 0), beam_width=2, search_width=2)
    assert not np.array_equal(base.cluster_label, ml_free_run.cluster_label), "'ml' and 'np' end in the same labels: the score is not exercised"
    assert 0 < ml_free_run.worst_rel_bound < 1e-4
    scores = [s for _, _, entries in ml_free_run.beam_trace for _, _, s in entries]
    assert len(scores) > 50 and all(s <= 0 for s in scores)


def test_follow_accepts_the_twins_own_trace(weights, furniture_room, ml_free_run):
    room = furniture_room
    got = beam_ml_ref.beam_room(room['points'], room['obj_id'], room['order'], weights, rng_ref.CounterStream(41, 0), beam_width=2,
                                search_width=2, scoring='ml', follow=ml_free_run.beam_trace)
    _same(got, ml_free_run)
    assert got.beam_trace == ml_free_run.beam_trace
    assert got.pairs_compared > 50 and got.pairs_undecided == 0


def test_follow_rejects_a_swapped_pair(weights, furniture_room, ml_free_run):
    room = furniture_room
    trace = copy.deepcopy(ml_free_run.beam_trace)
    for k, (seed, level, entries) in enumerate(trace):
        errs = ml_free_run.beam_trace_err[k]
        if len(entries) >= 2 and np.isfinite(entries[1][2]) and entries[0][2] - entries[1][2] > 100 * (errs[0] + errs[1]):
            entries[0], entries[1] = entries[1], entries[0]
            break
    else:
        pytest.fail('no record with two entries of clearly unequal score')
    with pytest.raises(beam_ml_ref.FollowError, match='seed %d level %d: consecutive entries' % (seed, level)):
        beam_ml_ref.beam_room(room['points'], room['obj_id'], room['order'], weights, rng_ref.CounterStream(41, 0), beam_width=2,
                              search_width=2, scoring='ml', follow=trace)


def test_command_line_accepts_beam_with_scoring_ml(capsys):
    import region_grow
    args = region_grow.parse_args(['--beam', '2', '--search-width', '2', '--scoring', 'ml'])
    assert (args.beam, args.scoring) == (2, 'ml')
    assert region_grow.parse_args(['--restarts', '4', '--scoring', 'ml']).scoring == 'ml'
    for bad in (['--scoring', 'ml'], ['--beam', '2', '--scoring', 'ml', '--rng', 'legacy'], ['--beam', '2', '--scoring', 'ml', '--restarts', '3']):
        with pytest.raises(SystemExit):
            region_grow.parse_args(bad)
    capsys.readouterr()
