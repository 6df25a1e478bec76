"""CPU: the NumPy restatement of the benchmarks.py baselines (tests/baselines_ref.py) against the reference script's own labels and
metric lines (tests/golden/baselines_ref_cpu.npz), the default thresholds, the new C-ABI exports and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO
import baselines_ref as R
from learn_region_grow_amd import baselines, metrics

MODES = ('normal', 'curvature', 'color', 'feature', 'smoothness')
ROOMS = (0, 1, 2)


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'baselines_ref_cpu.npz'))


@pytest.fixture(scope='module')
def rooms(golden):
    # the raw rooms are regenerated from their seeds; the digest the golden was made with pins them
    rooms = R.golden_rooms()
    assert R.rooms_digest(rooms) == str(golden['rooms_digest'])
    return rooms


@pytest.fixture(scope='module')
def feats(rooms):
    return {r: R.features(rooms[r]) for r in ROOMS}


@pytest.mark.parametrize('mode', MODES)
def test_restatement_equals_reference(golden, rooms, feats, mode):
    t = tuple(golden[mode + '__thresholds'])
    assert t == baselines.default_thresholds(mode, '5')
    for r in ROOMS:
        lab = R.segment(feats[r], mode, t)
        assert np.array_equal(lab, golden['%s__label%d' % (mode, r)]), (mode, r)
        obj = rooms[r][feats[r]['equalized_idx'], 6].astype(int)
        assert metrics.room_line('5', r, metrics.room_metrics(obj, lab)) == str(golden[mode + '__room_lines'][r])


def test_literal_smoothness_dfs_equals_reference(golden, feats):
    # the sparse room through the whole of :380-405 literally (every seed by DFS), not only the replayed components
    lab = R.segment_literal_smoothness(feats[2], 0.98)
    assert np.array_equal(lab, golden['smoothness__label2'])


def test_smoothness_golden_needs_duplicate_counting(golden, feats):
    # sizing a smoothness region by its distinct points instead of len(C) gives another answer on the golden
    differs = [r for r in ROOMS if not np.array_equal(R.segment(feats[r], 'smoothness', (0.98, 0, 0), distinct_only=True),
                                                       golden['smoothness__label%d' % r])]
    assert differs
    lab = golden['smoothness__label2']
    assert (np.unique(lab[lab > 0], return_counts=True)[1] <= 10).any()


def test_default_thresholds():
    assert baselines.default_thresholds('normal') == (0.99, 0.0, 0.0)
    assert baselines.default_thresholds('curvature') == (0.01, 0.0, 0.0)
    assert baselines.default_thresholds('color') == (0.005, 0.0, 0.0)
    assert baselines.default_thresholds('feature') == (0.98, 0.1, 0.1)
    assert baselines.default_thresholds('smoothness') == (0.98, 0.0, 0.0)
    assert baselines.default_thresholds('smoothness', 'scannet') == (0.985, 0.0, 0.0)
    assert baselines.MODES == MODES
    with pytest.raises(ValueError):
        baselines.default_thresholds('edge')


def test_capi_exports():
    from learn_region_grow_amd import _lib
    for name in ('lrg_baseline_workspace_bytes', 'lrg_baseline_segment', 'lrg_baseline_status'):
        assert name in _lib.EXPORTS
    assert 'lrg_baselines.hip' in _lib.SOURCES
    if os.path.exists(_lib.LIB_PATH):
        out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
        for name in ('lrg_baseline_workspace_bytes', 'lrg_baseline_segment', 'lrg_baseline_status'):
            assert ' T %s\n' % name in out
    header = open(os.path.join(REPO, 'include', 'lrg_hip.h')).read()
    assert 'int lrg_baseline_segment(' in header and '#define LRG_BASELINE_MAX_MIN_CLUSTER 64' in header


def test_cli_help():
    out = subprocess.run([sys.executable, os.path.join(REPO, 'baselines.py'), '--help'], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    for flag in ('--mode', '--area', '--h5', '--threshold', '--resolution', '--save', '--room-names', '--max-rooms', '--device'):
        assert flag in out.stdout
