"""CPU: the beam search's queue selection (csrc/lrg_beam_select.h, what lrg_beam_advance_kernel calls) over the fixed table of
tools/beam_select_table.hip -- a host program, no kernel, no HIP call -- against Python's sorted(), the reference's own selection
(test_beam_search.py:282): the best BEAM_WIDTH updated children by score, descending and stable, the emptied masks dropped afterwards."""
import os
import subprocess

import pytest

from conftest import REPO

SRC = os.path.join(REPO, 'tools', 'beam_select_table.hip')
TOOL = os.path.join(REPO, 'tools', 'build', 'beam_select_table')
HEADER = os.path.join(REPO, 'learn_region_grow_amd', 'csrc', 'lrg_beam_select.h')


@pytest.fixture(scope='module')
def table():
    """{name: case} from the tool's output; the tool is built on demand with the library's compiler and flags."""
    from learn_region_grow_amd import _lib
    if not os.path.exists(TOOL) or os.path.getmtime(TOOL) < max(os.path.getmtime(d) for d in (SRC, HEADER)):
        os.makedirs(os.path.dirname(TOOL), exist_ok=True)
        hipcc, flags = _lib.hipcc_and_flags()
        cmd = [hipcc] + flags + [SRC, '-o', TOOL]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        assert done.returncode == 0, '%s\n%s' % (' '.join(cmd), done.stderr)
    done = subprocess.run([TOOL], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert done.returncode == 0, done.stderr
    out = {}
    for line in done.stdout.splitlines():
        name, ml, bw, sw, upd, size, score, best, kept = line.split('|')
        ints = lambda s: [int(v) for v in s.split(',')] if s else []
        assert name not in out
        out[name] = dict(ml=int(ml), bw=int(bw), sw=int(sw), updated=ints(upd), size=ints(size),
                         score=[float(v) for v in score.split(',')] if score else [], best=ints(best), kept=ints(kept))
    return out


def python_selection(c):
    """Q = sorted(newQ, key=score, reverse=True)[:BEAM_WIDTH]; then without the emptied masks (oracle/beam_ref.py:139-140)"""
    key = c['score'] if c['ml'] else c['size']
    new_q = [i for i, u in enumerate(c['updated']) if u == 1]                 # appended in (qid, search id) order (:276)
    best = sorted(new_q, key=lambda i: key[i], reverse=True)[:c['bw']]
    return best, [i for i in best if c['size'][i] > 0]


def test_every_case_is_pythons_selection(table):
    assert len(table) > 400
    for name, c in table.items():
        assert len(c['updated']) == len(c['size']) == len(c['score']) <= 64 and 1 <= c['bw'] <= 16 and c['bw'] * c['sw'] <= 64, name
        best, kept = python_selection(c)
        assert (c['best'], c['kept']) == (best, kept), name
    sweep = [c for name, c in table.items() if name.startswith('sweep_')]
    # the sweep holds what it is for: both scores, ties among the chosen, more candidates than places, emptied masks chosen, -inf chosen
    assert sum(c['ml'] for c in sweep) > 100 and sum(1 - c['ml'] for c in sweep) > 100
    assert sum(1 for c in sweep if sum(u == 1 for u in c['updated']) > c['bw']) > 50
    assert sum(1 for c in sweep if len(c['kept']) < len(c['best'])) > 50
    assert sum(1 for c in sweep if c['ml'] and any(c['score'][i] == float('-inf') for i in c['best'])) > 20


def test_named_cases(table):
    t = table
    assert t['np_size_ties']['best'] == [1, 3, 6] == t['np_size_ties']['kept']            # 9, 9, 9 in child order; child 8 (also 9) is out
    assert t['np_empties_last']['best'] == [1, 3, 0] and t['np_empties_last']['kept'] == [1, 3]
    assert t['ml_exact_tie']['best'] == [1, 2]                                             # three -0.25: the first two in child order
    assert t['ml_minus_inf']['best'] == [1, 0, 2] == t['ml_minus_inf']['kept']             # -inf orders last, ties among -inf stable
    assert t['ml_all_minus_inf']['best'] == [0, 1]
    assert t['ml_more_than_beam']['best'] == [1, 3]
    assert t['ml_empty_mask_on_top']['best'] == [0, 1] and t['ml_empty_mask_on_top']['kept'] == [1]      # a place taken, then dropped
    assert t['ml_only_empties_survive']['best'] == [0, 1] and t['ml_only_empties_survive']['kept'] == []
    for name in ('no_candidate_np', 'no_candidate_ml', 'no_children'):
        assert t[name]['best'] == [] == t[name]['kept']
    assert t['beam_1']['best'] == [1]
    for name in ('bw16_sw4_ml', 'bw16_sw4_np'):
        assert (t[name]['bw'], t[name]['sw'], len(t[name]['updated']), len(t[name]['best'])) == (16, 4, 64, 16)
    assert 0 in [t['bw16_sw4_ml']['size'][i] for i in t['bw16_sw4_ml']['best']]            # an emptied mask among the sixteen
