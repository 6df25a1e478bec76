"""Host: the rooms and hand-made results of tests/beam_rooms.py do what the GPU beam tests rely on (tests/test_gpu_beam_shapes.py, the
searches above 3 x 3 of tests/test_gpu_beam_ml.py), so that those cannot pass for the wrong reason.  oracle/lrgnet_ref.py is the network:
no GPU.  And the NumPy selection those tests compare with is lrg_beam_select's (csrc/lrg_beam_select.h) on every 64-slot pattern, through
the host table tool."""
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO

import beam_ml_ref
import beam_rooms
from learn_region_grow_amd import synthetic
from oracle import grow_ref, rng_ref

WEIGHT_KW = dict(seed=0, gain=2.0, bias_std=0.2, add_bias_shift=0.0, rmv_bias_shift=-3.0)
SRC = os.path.join(REPO, 'tools', 'beam_select_table.hip')
TOOL = os.path.join(REPO, 'tools', 'build', 'beam_select_table')
HEADER = os.path.join(REPO, 'learn_region_grow_amd', 'csrc', 'lrg_beam_select.h')


@pytest.fixture(scope='module')
def weights():
    return synthetic.make_synthetic_weights(**WEIGHT_KW)


def _search(room, weights, BW, SW, ni, nn, scoring, seed=21, follow=None):
    return beam_ml_ref.beam_room(room['points'], room['obj_id'], room['order'], weights, rng_ref.CounterStream(seed, room['room_id']),
                                 beam_width=BW, search_width=SW, num_inlier=ni, num_neighbor=nn, policy='net', scoring=scoring, follow=follow)


def test_rooms_are_equalised():
    for room, n in ((beam_rooms.strip_room(), 199), (beam_rooms.ml_crop_room(), 290), (beam_rooms.tiny_room(1, 1), 1), (beam_rooms.tiny_room(2, 2), 2),
                    (beam_rooms.below_threshold_room(), 19)):
        assert room['points'].shape == (n, 13) and room['points'].dtype == np.float32
        assert len(np.unique(grow_ref.pack_voxels(grow_ref.voxelize(room['points'][:, :3], beam_rooms.RES)))) == n
        assert sorted(np.asarray(room['order']).tolist()) == list(range(n))
    crop = beam_rooms.ml_crop_room()
    assert np.bincount(crop['obj_id'])[beam_rooms.ML_CROP_OBJECT] == 70 and len(np.unique(crop['obj_id'])) == 5


def _commits(res):
    """(regions that ended by a dry queue, by the stall rule): a stalled head leaves a last record with survivors"""
    last = {}
    for seed, _, entries in res.beam_trace:
        last[seed] = entries
    dry = sum(1 for r in res.regions if not [x for x in last[r['seed']] if x[1] > 0])
    return dry, len(res.regions) - dry


@pytest.mark.parametrize('BW,SW', [(4, 4), (3, 3)])
def test_strip_room_fills_the_queue(weights, BW, SW):
    """The strip room under the Bernoulli policy: the queue reaches beam_width and there are regions above and below the cluster
    threshold.  Every region there ends by a dry queue -- the largest mask always reaches further -- so the searches also take the crop,
    where heads stall (below).  (16 x 4, 8 x 8 and 1 x 64 cost the host 2 to 5 thousand evaluations: the GPU tests assert the same of their runs.)"""
    res = _search(beam_rooms.strip_room(), weights, BW, SW, 128, 128, 'np')
    assert max(len(e) for _, _, e in res.beam_trace) == BW
    assert _commits(res) == (len(res.regions), 0)
    assert any(r['labeled'] for r in res.regions) and any(not r['labeled'] for r in res.regions)
    assert sum(r['points'] for r in res.regions) == 199


def test_crop_room_stalls(weights):
    """Scoring 'np', one child per parent: the crop's regions end both ways, labelled and not"""
    res = _search(beam_rooms.ml_crop_room(), weights, 16, 1, 128, 128, 'np')
    dry, stall = _commits(res)
    assert dry > 0 and stall > 0
    assert any(r['labeled'] for r in res.regions) and any(not r['labeled'] for r in res.regions)


@pytest.mark.parametrize('BW,SW,ni,nn', [(8, 4, 128, 128), (4, 4, 64, 128)])
def test_ml_crop_self_follow(weights, BW, SW, ni, nn):
    """The crop under --scoring ml, the twin following its own trace: within the limits its choice was made by (at most 5 % of the pairs
    undecided, bound below 1e-3 relative, about 2 k evaluations), and the figures tests/beam_rooms.py records."""
    room = beam_rooms.ml_crop_room()
    own = _search(room, weights, BW, SW, ni, nn, 'ml')
    res = _search(room, weights, BW, SW, ni, nn, 'ml', follow=own.beam_trace)
    print('%d x %d, %d/%d: %d evaluations, %d pairs, %d undecided, bound %.2g' % (BW, SW, ni, nn, own.total_steps, res.pairs_compared,
                                                                                  res.pairs_undecided, res.worst_rel_bound))
    assert res.pairs_compared > 50 and res.pairs_undecided <= 0.05 * res.pairs_compared
    assert res.worst_rel_bound < 1e-3 and own.total_steps <= 2000
    evals, pairs, undecided, bound = beam_rooms.ML_CROP_FIGURES[(BW, SW, ni, nn, 21)]
    assert (own.total_steps, res.pairs_compared, res.pairs_undecided) == (evals, pairs, undecided) and res.worst_rel_bound <= 1.1 * bound
    assert max(len(e) for _, _, e in own.beam_trace) == BW
    dry, stall = _commits(own)
    assert dry > 0 and stall > 0
    # no emptied mask comes among the best in these searches: the direct tests of lrg_beam_advance (pattern 'ml_empty_on_top') stand for it
    assert not any(size == 0 for _, _, e in own.beam_trace for _, size, _ in e)


def test_scripts_reach_what_they_are_for():
    """The hand-made levels of the direct lrg_beam_advance test on the model alone: the widest level has every child of the group, both
    kinds of commit occur, labelled and unlabelled regions, and under 'ml' an emptied mask and a -inf score among the best."""
    room = beam_rooms.strip_room([(8, 300), (8, 301)], room_id=44)
    n = len(room['points'])
    for BW, SW in beam_rooms.GROUP_SHAPES:
        for ml in (0, 1):
            m = beam_rooms.GroupModel(room, 0, BW, SW, ml)
            rs = np.random.RandomState(100 * BW + SW + ml)
            m.advance()
            widest, short = 0, False
            for pattern in beam_rooms.advance_script(BW, SW, ml):
                children = beam_rooms.child_results(pattern, len(m.Q) * SW, BW, SW, n, (m.seq_mn, m.seq_mx), rs)
                widest = max(widest, len(children))
                assert len(set(c['mask'].tobytes() for c in children if c['size'])) == sum(1 for c in children if c['size'])      # distinct masks
                m.advance(children)
                short |= pattern == 'ml_empty_on_top' and 0 < len(m.Q) < min(BW, len(children)) and m.level > 0
                assert not m.done
            assert widest == (BW * SW if SW > 1 else 1)
            assert 'dry' in m.commits and 'stall' in m.commits
            assert any(r[4] for r in m.region_log) and any(not r[4] for r in m.region_log)
            if ml:
                assert any(any(x[1] == 0 for x in e) for _, _, e in m.trace) and any(any(x[2] == -np.inf for x in e) for _, _, e in m.trace)
                assert short or min(BW, SW) == 1          # an emptied mask took a place: the queue came out shorter (one place or one child: dry)


def test_selection_is_lrg_beam_select(tmp_path):
    """beam_rooms.select (Python's sorted, then without the emptied masks) against lrg_beam_select on every pattern at every group shape"""
    from learn_region_grow_amd import _lib
    if not os.path.exists(TOOL) or os.path.getmtime(TOOL) < max(os.path.getmtime(d) for d in (SRC, HEADER)):
        os.makedirs(os.path.dirname(TOOL), exist_ok=True)
        hipcc, flags = _lib.hipcc_and_flags()
        cmd = [hipcc] + flags + [SRC, '-o', TOOL]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        assert done.returncode == 0, '%s\n%s' % (' '.join(cmd), done.stderr)
    cases = beam_rooms.g64_cases()
    path = str(tmp_path / 'cases.txt')
    with open(path, 'w') as f:
        for name, ml, BW, SW, upd, size, score in cases:
            f.write('%s|%d|%d|%d|%s|%s|%s\n' % (name, ml, BW, SW, ','.join(map(str, upd)), ','.join(map(str, size)),
                                               ','.join('-inf' if x == -np.inf else repr(float(x)) for x in score) if ml else ''))
    done = subprocess.run([TOOL, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert done.returncode == 0, done.stderr
    lines = done.stdout.splitlines()
    assert len(lines) == len(cases) == 7 * (7 + 13)
    ints = lambda s: [int(v) for v in s.split(',')] if s else []
    full = 0
    for line, (name, ml, BW, SW, upd, size, score) in zip(lines, cases):
        got = line.split('|')
        assert got[0] == name and ints(got[4]) == upd and ints(got[5]) == size
        best, kept = beam_rooms.select(upd, size, score, ml, BW)
        assert (ints(got[7]), ints(got[8])) == (best, kept), name
        full += len(upd) == 64
    assert full == 4 * 20          # 16 x 4, 8 x 8, 4 x 16 and 1 x 64 at all 64 slots
