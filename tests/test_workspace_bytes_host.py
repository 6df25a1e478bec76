"""CPU: the workspace sizes of the batched off-hot-path modules (baselines, FPFH, MCPNet, edge, metrics, preprocessing) are the ones
recorded in tests/golden/workspace_bytes.json before their layouts moved onto the shared arena, slot-count and scan-block helpers
(csrc/lrg_common.h, lrg_room_hash.h).  Callers keep workspaces across library versions by size alone, so a size is part of the ABI."""
import ctypes
import json
import os

from conftest import REPO

SHAPES = [(0, 1), (1, 1), (300, 1), (21000, 70), (210000, 1)]      # (points, rooms)
MIN_CLUSTER, SEARCH_CAP, GT_ROWS, CLUSTERS = 10, 4096, 3, 5


def _starts(total, rooms):
    """rooms + 1 bounds of rooms of (nearly) equal size"""
    return (ctypes.c_int32 * (rooms + 1))(*[total * r // rooms for r in range(rooms + 1)])


def workspace_bytes(lib):
    """{entry point: [[points, rooms, bytes], ...]}; 0 is the entry's refusal (preprocessing and metrics take no empty room)"""
    out = {}

    def put(name, n, r, v):
        out.setdefault(name, []).append([n, r, int(v)])
    for n, r in SHAPES:
        put('lrg_baseline_workspace_bytes', n, r, lib.lrg_baseline_workspace_bytes(n, r, MIN_CLUSTER))
        put('lrg_baseline_fpfh_workspace_bytes', n, r, lib.lrg_baseline_fpfh_workspace_bytes(n, r, MIN_CLUSTER))
        put('lrg_fpfh_workspace_bytes', n, r, lib.lrg_fpfh_workspace_bytes(n, r, 0))
        put('lrg_fpfh_workspace_bytes:lists', n, r, lib.lrg_fpfh_workspace_bytes(n, r, 1))
        put('lrg_mcp_workspace_bytes', n, r, lib.lrg_mcp_workspace_bytes(n, r))
        put('lrg_edge_workspace_bytes', n, r, lib.lrg_edge_workspace_bytes(n, r, MIN_CLUSTER, SEARCH_CAP))
        ncl = (ctypes.c_int32 * r)(*[CLUSTERS] * r)
        put('lrg_metrics_batch_workspace_bytes', n, r, lib.lrg_metrics_batch_workspace_bytes(_starts(n, r), _starts(GT_ROWS * r, r), ncl, r))
        put('lrg_preprocess_batch_workspace_bytes', n, r, lib.lrg_preprocess_batch_workspace_bytes(_starts(n, r), r))
        if r == 1:
            put('lrg_preprocess_workspace_bytes', n, r, lib.lrg_preprocess_workspace_bytes(n))
    return out


def test_workspace_bytes_are_the_recorded_ones(hip_lib):
    want = json.load(open(os.path.join(REPO, 'tests', 'golden', 'workspace_bytes.json')))
    got = workspace_bytes(hip_lib)
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert got[name] == want[name], name
    # every module is exercised: a size of 0 only where the entry refuses the shape
    for name, rows in want.items():
        for n, r, v in rows:
            refused = n == 0 and ('preprocess' in name or 'metrics' in name)
            assert (v == 0) == refused, (name, n, r, v)
