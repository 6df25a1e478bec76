"""CPU: the register-tile CUs by role (csrc/lrg_async_plan.h: lrg_rt_role; the plan field rt_head_every, the switch LRG_ASYNC_RT_HEAD_EVERY) over the sweep of
tools/async_plan_table.hip, line for line against tests/golden/async_roles_table.txt.

`async_plan_table --roles` makes, for every case of the sweep, the plan with the switch unset, 0, 2, 3, 4 and 64 and counts -- with the functions the worker
kernel itself reads -- the CUs of each role, the teams on each ring and the fewest teams of either ring on 8 consecutive worker workgroups (one per XCD).  Without
the flag the tool prints what it always did (tests/test_async_plan.py).  A change that is meant regenerates the file:
    tools/build/async_plan_table --roles > tests/golden/async_roles_table.txt
"""
import os
import subprocess

import pytest

from conftest import GOLDEN, REPO

SRC = os.path.join(REPO, 'tools', 'async_plan_table.hip')
TOOL = os.path.join(REPO, 'tools', 'build', 'async_plan_table')
GOLDEN_ROLES = os.path.join(GOLDEN, 'async_roles_table.txt')
ASKED = ['unset', '0', '2', '3', '4', '64']


@pytest.fixture(scope='module')
def roles(hip_lib):
    """The lines of `async_plan_table --roles` (the tool is built as tests/test_async_plan.py builds it) and its exit code"""
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
    done = subprocess.run([TOOL, '--roles'], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert done.returncode in (0, 1), done.stderr
    return done.stdout.splitlines(), done.returncode, done.stderr


def reg_rows(lines):
    """(label, asked, rt_head_every, rt_bb_every, [CUs MIXED, BRANCH2, BRANCH1, HEAD2], [teams ring 0, ring 1, fill-in], [fewest ring 0, ring 1 on 8]) of the register-tile rows"""
    for line in lines[1:]:
        part = line.split('|')
        if part[1] != '-':
            he, bb = (int(v) for v in part[2].split())
            yield part[0], part[1], he, bb, [int(v) for v in part[3].split()], [int(v) for v in part[4].split()], [int(v) for v in part[5].split()]


def test_roles_are_the_golden_ones(roles):
    lines, rc, err = roles
    assert rc == 0, err      # (the tool's own checks: no empty ring, never both switches, no roles without register tiles)
    want = open(GOLDEN_ROLES).read().splitlines()
    assert os.path.getsize(GOLDEN_ROLES) <= 256 * 1024
    differ = [(w, g) for w, g in zip(want, lines) if w != g]
    assert len(want) == len(lines) and not differ, '%d lines against %d, %d differ:\n%s' % (
        len(lines), len(want), len(differ), '\n'.join('  want %s\n  got  %s' % d for d in differ[:20]))


def test_no_granted_row_has_an_empty_ring(roles):
    rows = list(reg_rows(roles[0]))
    assert len(rows) >= 6 * 300 and {r[1] for r in rows} == set(ASKED)
    for label, asked, he, bb, cus, teams, least in rows:
        assert teams[0] > 0 and teams[1] > 0, (label, asked)
        assert sum(cus) * 2 >= sum(teams) and sum(cus) >= 24, (label, asked)
        if he:
            # by role: every CU is BRANCH1 or HEAD2, one stripe of 8 in `he` is HEAD2, and `he` was kept within 2 .. (worker workgroups) / 8
            assert cus[0] == 0 and cus[1] == 0 and cus[3] > 0 and cus[2] > 0, (label, asked)
            assert 2 <= he <= sum(cus) // 8 and cus[3] == 8 * (sum(cus) // 8 // he), (label, asked)
            assert teams == [cus[2], 2 * cus[3], 0], (label, asked)
        else:
            assert cus[2] == 0 and cus[3] == 0, (label, asked)
            assert least[0] >= 8, (label, asked)      # (every CU has a branch team)


def test_head_every_and_bb_every_never_combine(roles):
    asked_both = 0
    for label, asked, he, bb, cus, teams, least in reg_rows(roles[0]):
        assert not (he and bb), (label, asked)
        asked_both += 'sw.rt_bb_every=2' in label and asked in ('2', '3', '4', '64')
    assert asked_both == 8      # (68 and 136 slots with LRG_ASYNC_RT_BB_EVERY=2 and the new switch at a non-zero value: rt_bb_every gives way)
    by = {(r[0], r[1]): r for r in reg_rows(roles[0])}
    assert by[('n136/sw.rt_bb_every=2', '0')][3] == 2 and by[('n136/sw.rt_bb_every=2', '3')][2:4] == (3, 0)
    # the switch at 0 or unset above the automatic range: today's plan, every fourth CU with two branch teams from 120 slots
    assert by[('n148w0u0t0', '0')][3] == 4 and by[('n176w0u0t0', 'unset')][3] == 4 and by[('n128w0u0t0', 'unset')][2] == 0


def test_the_switch_is_asked_for_what_it_says(roles):
    by = {(r[0], r[1]): r for r in reg_rows(roles[0])}
    # 192 worker workgroups: 2 -> 96 + 96 CUs, 3 -> 128 + 64, 4 -> 144 + 48, 64 -> kept to 24: one stripe of 8 CUs
    assert [by[('n47w0u0t0', a)][4][2:] for a in ('2', '3', '4', '64')] == [[96, 96], [128, 64], [144, 48], [184, 8]]
    assert by[('n47w0u0t0', '64')][2] == 24 and by[('n47w0u0t0', '0')][4] == [192, 0, 0, 0]
    # fill-in teams and team head tiles keep every CU mixed, whatever the switch
    for label in ('n68/fill/fill_wgs=8/w0', 'n68/sw.rt_team_heads=1'):
        assert all(by[(label, a)][2] == 0 for a in ASKED), label


def test_no_lite2_or_other_heads_row_has_roles(roles):
    plain = {}
    for line in roles[0][1:]:
        part = line.split('|')
        if part[1] == '-':
            plain[part[0]] = [int(v) for v in part[2].split()]
    reg = {r[0] for r in reg_rows(roles[0])}
    others = [k for k in plain if k.startswith(('lite2/', 'h128/', 'h256x64/'))]
    assert len(others) >= 75 and {'lite2/n84', 'h128/n68/w1', 'h256x64/n176'} <= set(others)
    assert not [k for k in reg if k.startswith(('lite2/', 'h128/', 'h256x64/'))]
    for label, values in plain.items():
        assert values == [0] * 6, label
