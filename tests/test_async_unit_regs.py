"""CPU: the form of the pooled-product units (csrc/lrg_async_plan.h: the plan field unit_regs, the switch LRG_ASYNC_UNIT_REGS) over the sweep of
tools/async_plan_table.hip, line for line against tests/golden/async_unit_regs_table.txt.

`async_plan_table --unit-regs` makes, for every granted case of the sweep, the plan with the switch unset, 0 and 1 and prints the units, the half-teams, the three
plans' unit_regs and their LDS.  Without the flag the tool prints what it always did, byte for byte (tests/test_async_plan.py compares that with its own golden
file; here the two are compared once more, so that this file stands alone).  A change that is meant regenerates the file:
    tools/build/async_plan_table --unit-regs > tests/golden/async_unit_regs_table.txt
"""
import os
import subprocess

import pytest

from conftest import GOLDEN, REPO

SRC = os.path.join(REPO, 'tools', 'async_plan_table.hip')
TOOL = os.path.join(REPO, 'tools', 'build', 'async_plan_table')
GOLDEN_UNITS = os.path.join(GOLDEN, 'async_unit_regs_table.txt')


@pytest.fixture(scope='module')
def tool(hip_lib):
    """The table tool, built as tests/test_async_plan.py builds it"""
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
    return TOOL


@pytest.fixture(scope='module')
def rows(tool):
    done = subprocess.run([tool, '--unit-regs'], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert done.returncode == 0, done.stderr      # (the tool's own checks: never without units, never for other heads, the switch moves nothing else)
    return done.stdout.splitlines()


def parsed(lines):
    """label -> (gemv_units, unit_pairs, [unit_regs unset, 0, 1], [lds unset, 0, 1])"""
    out = {}
    for line in lines[1:]:
        label, units, regs, lds = line.split('|')
        u, p = (int(v) for v in units.split())
        out[label] = (u, p, [int(v) for v in regs.split()], [int(v) for v in lds.split()])
    return out


def test_table_is_the_golden_one(rows):
    want = open(GOLDEN_UNITS).read().splitlines()
    assert os.path.getsize(GOLDEN_UNITS) <= 256 * 1024
    differ = [(w, g) for w, g in zip(want, rows) if w != g]
    assert len(want) == len(rows) and not differ, '%d lines against %d, %d differ:\n%s' % (
        len(rows), len(want), len(differ), '\n'.join('  want %s\n  got  %s' % d for d in differ[:20]))


def test_default_table_is_byte_identical(tool):
    done = subprocess.run([tool], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert done.returncode == 0, done.stderr
    assert done.stdout == open(os.path.join(GOLDEN, 'async_plan_table.txt'), 'rb').read()


def test_the_form_goes_with_the_units_and_the_papers_heads(rows):
    by = parsed(rows)
    assert len(by) >= 1500
    for label, (units, pairs, regs, lds) in by.items():
        assert regs[1] == 0, label                                     # forced off
        assert lds[0] == lds[1] == lds[2], label                       # the FIFO lies inside the units' LDS: the plan's LDS does not move
        if label.startswith(('lite2/', 'h128/')) or not units:
            assert regs == [0, 0, 0], label
        else:
            assert units == 16 and regs[2] == 1, label                 # forced on wherever the units are
    # the paper's network: on with the units below and above the slot count from which the half-teams are chosen; the fields of the older forms keep their values
    assert by['n47w0u0t0'][:3] == (16, 0, [1, 0, 1]) and by['n128w0u0t0'][:3] == (16, 1, [1, 0, 1]) and by['n68/gemv_units=1'][:3] == (16, 0, [1, 0, 1])
    assert by['n47w0u-1t0'][0] == 0 and by['lite2/n84'][0] == 4 and by['n68/pool_rows/gemv_units=1'][2] == [1, 0, 1]
    assert by['h256x64/n84'][2] == [1, 0, 1]                           # (the paper's first head layer, another second width: the same pooled product)
