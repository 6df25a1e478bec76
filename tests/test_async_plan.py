"""CPU: the launch plan of lrg_grow_async (csrc/lrg_async_plan.inl) over the fixed sweep of tools/async_plan_table.hip -- no kernel, no HIP
call, made-up addresses -- line for line against tests/golden/async_plan_table.txt.

The golden file holds the plans as they were before the plan became a file and steps of its own: a change to a decision of the plan moves
rows here, and the rows name the launches it changes.  A change that is meant regenerates the file:
    tools/build/async_plan_table > tests/golden/async_plan_table.txt        (--full prints every field of every plan)
"""
import os
import subprocess

import pytest

from conftest import GOLDEN, REPO

SRC = os.path.join(REPO, 'tools', 'async_plan_table.hip')
TOOL = os.path.join(REPO, 'tools', 'build', 'async_plan_table')
GOLDEN_TABLE = os.path.join(GOLDEN, 'async_plan_table.txt')
SLOTS = [1, 16, 17, 24, 25, 46, 47, 83, 84, 96, 97, 119, 120, 128, 129, 148, 149, 176, 177, 200, 201, 224, 272, 400, 480, 544, 2048, 2049,
         4096, 4097]


@pytest.fixture(scope='module')
def table(hip_lib):
    """The tool's output lines; the tool is built on demand with the library's compiler and flags and linked against the library."""
    from learn_region_grow_amd import _lib
    csrc = os.path.join(REPO, 'learn_region_grow_amd', 'csrc')
    deps = [SRC, os.path.join(REPO, 'include', 'lrg_hip.h')] + [os.path.join(csrc, f) for f in ('lrg_async_plan.h', 'lrg_fused.h', 'lrg_common.h')]
    if not os.path.exists(TOOL) or os.path.getmtime(TOOL) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(TOOL), exist_ok=True)
        hipcc, flags = _lib.hipcc_and_flags()
        libdir = os.path.dirname(_lib.LIB_PATH)
        cmd = [hipcc] + flags + [SRC, '-o', TOOL, '-L', libdir, '-l:' + os.path.basename(_lib.LIB_PATH), '-Wl,-rpath,' + libdir]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        assert done.returncode == 0, '%s\n%s' % (' '.join(cmd), done.stderr)
    done = subprocess.run([TOOL], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    # (non-zero: the sweep no longer holds what it must -- every refusal code, the paper-shape kernels on the paper's network only, at most a fifth refusals)
    assert done.returncode == 0, done.stderr
    return done.stdout.splitlines()


def granted(table):
    """(label, {column: value}) of the granted cases"""
    columns = table[0].split('|')[2].split()
    for line in table[1:]:
        part = line.split('|')
        if not line.startswith('Q ') and part[1] == '0':
            values = []
            for v in part[2].split():      # (0*k: a run of k zeros)
                values += [0] * int(v[2:]) if v.startswith('0*') else [int(v)]
            assert len(values) == len(columns), line
            yield part[0], dict(zip(columns, values))


def test_plans_are_the_golden_ones(table):
    want = open(GOLDEN_TABLE).read().splitlines()
    assert os.path.getsize(GOLDEN_TABLE) <= 256 * 1024
    got_by, want_by = ({line.split('|')[0]: line for line in t} for t in (table, want))
    moved = [k for k in want_by if k in got_by and got_by[k] != want_by[k]]
    gone, new = [k for k in want_by if k not in got_by], [k for k in got_by if k not in want_by]
    assert not (moved or gone or new), '%d cases differ from tests/golden/async_plan_table.txt, %d are missing, %d are new:\n%s' % (
        len(moved), len(gone), len(new), '\n'.join(['  want %s\n  got  %s' % (want_by[k], got_by[k]) for k in moved[:20]] + ['  missing %s' % k for k in gone[:20]] +
                                                   ['  new %s' % k for k in new[:20]]))
    assert table == want      # (and in the same order)


def test_queue_covers_the_rings_the_plan_addresses(table, hip_lib):
    """LRG_AQ_WAVE_RING(A, 8), the end of the last ring (the largest over the granted plans of a slot count), is inside lrg_grow_async_queue_bytes"""
    seen = {}
    for line in table:
        if line.startswith('Q '):
            n, ring_end, words = (int(v) for v in line.split()[1:])
            assert words * 4 == hip_lib.lrg_grow_async_queue_bytes(n)
            assert 0 < ring_end <= words, '%d slots: the rings end at word %d of a queue of %d' % (n, ring_end, words)
            seen[n] = ring_end
    assert set(SLOTS) <= set(seen)


def test_paper_shape_kernels_are_granted_to_the_paper_shape_only(table):
    """lrg_async_gemv_unit2 (half-teams in the pooled-product units) is written for 1024 pooled features and lrg_team_head_tile_reg (the head tiles of a
    register-tile launch) for the heads 256, 128, 2.  By label prefix: no lite-2 row (512 pooled features) has unit_pairs, forced rows included; no row of the
    heads 128, 64, 2 or 256, 64, 2 on the paper's branches has register tiles or any other two-kernel launch (worker_wgs, wave_wgs) -- and the units those
    networks keep stop at the one-kernel launch's 148 slots, not at the register tiles' 176.  The paper's own rows still have both."""
    rows = list(granted(table))
    lite2 = [(k, v) for k, v in rows if k.startswith('lite2/')]
    heads = [(k, v) for k, v in rows if k.startswith('h128/') or k.startswith('h256x64/')]
    assert dict(rows)['plan/n_head=2']['reg_tiles'] == 0      # (a head stack of two layers, 256 -> 2, at 68 slots)
    assert len(lite2) >= 25 and len(heads) >= 50      # (the thirty slot counts of the sweep, less the few that are refused)
    assert {'lite2/n84', 'lite2/n148', 'lite2/n68/sw.unit_pairs=1', 'lite2/n136/sw.unit_pairs=1'} <= {k for k, _ in lite2}
    assert {'h128/n1', 'h128/n68/sw.unit_pairs=1', 'h128/n68/w1', 'h256x64/n1', 'h256x64/n176', 'h256x64/n68/w1'} <= {k for k, _ in heads}
    for label, v in lite2:
        assert v['unit_pairs'] == 0, label
        assert v['reg_tiles'] == 0 and v['worker_wgs'] == 0, label
    assert any(v['gemv_units'] == 4 for k, v in lite2 if k in ('lite2/n84', 'lite2/n148'))      # (the units themselves stay: four wavefronts per task)
    for label, v in heads:
        assert v['reg_tiles'] == 0 and v['worker_wgs'] == 0 and v['wave_wgs'] == 0, label
        n = int(label.split('/')[1][1:])
        assert v['gemv_units'] == 0 or n <= 148, label
    paper = dict(rows)
    assert paper['n47w0u0t0']['reg_tiles'] == 1 and paper['n128w0u0t0']['reg_tiles'] == 1 and paper['n128w0u0t0']['unit_pairs'] == 1


def test_both_kernels_lds_fits_a_cu(table):
    n = 0
    for label, v in granted(table):
        assert 0 < v['lds'] <= 160 * 1024 and 0 < v['worker_lds'] <= 160 * 1024, label
        n += 1
    assert n > 1500
