#!/usr/bin/env python3
"""Measure the edge-classifier baseline on the GPU (learn_region_grow_amd.edge) -> profiles/edge_bench.json.

The 68 Area-5-shaped rooms of the other baseline benches (synthetic.area5_shaped_room at AREA5_POINTS, 0.1 m) in one batch, the
classifier of tests/golden/edge5_weights.npz.  Device times by HIP events (warm-up, then repeats for at least --min-seconds):
lrg_edge_logits (init, insert, neighbours, the MLP), lrg_edge_sigmoid, lrg_edge_segment; the same four layers as torch float64
matmuls on the same F; rooms/s end to end for both sigmoid routes (room dicts in, labels out); the share of edges within 1e-9 of
a threshold; the largest visited set; searches and overflowed searches at several caps.

    python tools/edge_bench.py [--out profiles/edge_bench.json] [--rooms 68]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

FP64_VECTOR_TFLOPS = 78.6      # MI355X float64 vector peak, an FMA counted as two operations
MACS = 30 * 100 + 100 * 50 + 50 * 25 + 25


def timed(torch, fn, min_seconds):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    reps, total = 0, 0.0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    while total < min_seconds:
        k = max(1, reps)
        e0.record()
        for _ in range(k):
            fn()
        e1.record()
        e1.synchronize()
        total += e0.elapsed_time(e1) / 1e3
        reps += k
    return total / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'edge_bench.json'))
    ap.add_argument('--rooms', type=int, default=68)
    ap.add_argument('--min-seconds', type=float, default=1.0)
    args = ap.parse_args()
    import torch
    from scipy.special import expit
    from learn_region_grow_amd import _lib, baselines, edge, synthetic
    import baselines_ref
    import edge_ref
    lib = _lib.load()
    dev = torch.device('cuda:0')
    weights = edge_ref.golden_weights()
    model = edge.EdgeModelHIP(weights, device=dev)
    raw = [synthetic.area5_shaped_room(t, 1000 + i).astype(np.float32) for i, t in enumerate(synthetic.AREA5_POINTS[:args.rooms])]
    rooms = [baselines.room_features(r, need_normals=False, device=dev) for r in raw]
    pts, room_start, n = edge._batch(rooms, dev)
    R = len(rooms)
    rs = room_start.ctypes.data_as(ctypes.c_void_p)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = edge._ptr
    ws = torch.empty(lib.lrg_edge_workspace_bytes(n, R, 10, 1024), dtype=torch.uint8, device=dev)
    z = torch.empty((n, 13), dtype=torch.float64, device=dev)
    p = torch.empty_like(z)
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    stop = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty(R, dtype=torch.int32, device=dev)
    counters = torch.zeros(4, dtype=torch.int32, device=dev)
    res = ctypes.c_float(0.1)

    def run_logits():
        assert lib.lrg_edge_logits(P(pts), 6, rs, R, res, P(model.packed), P(ws), ws.numel(), P(z), None, None, st) == 0

    def run_sigmoid():
        assert lib.lrg_edge_sigmoid(P(z), z.numel(), P(p), st) == 0

    def run_segment(cap=1024, prepared=0):
        assert lib.lrg_edge_segment(P(pts), 6, rs, R, res, P(p), 0.99, 0.9, 10, cap, P(ws), ws.numel(), P(labels), P(counts), P(stop), P(counters),
                                    None, None, prepared, st) == 0
    out = dict(rooms=R, points=n)
    out['logits_s'] = timed(torch, run_logits, args.min_seconds)
    zh = z.cpu().numpy()
    edges = int((~np.isnan(zh)).sum())
    out['edges'] = edges
    out['logits_tflops'] = 2.0 * MACS * edges / out['logits_s'] / 1e12
    out['logits_share_of_fp64_vector_peak'] = out['logits_tflops'] / FP64_VECTOR_TFLOPS
    out['sigmoid_s'] = timed(torch, run_sigmoid, args.min_seconds)
    p.copy_(torch.from_numpy(expit(zh)).to(dev))                                 # the host route's p for the stages after it
    out['segment_s'] = timed(torch, run_segment, args.min_seconds)
    out['segment_prepared_s'] = timed(torch, lambda: run_segment(prepared=1), args.min_seconds)      # on the workspace lrg_edge_logits left
    out['by_cap'] = {}
    for cap in (32, 64, 128, 256, 512, 1024):
        run_segment(cap)
        torch.cuda.synchronize()
        dead, searches, over, largest = (int(x) for x in counters.cpu().numpy())
        out['by_cap'][str(cap)] = dict(dead_points=dead, searches=searches, overflowed=over)
    out['largest_visited_set'] = largest                                          # of the run at the default cap, where nothing overflowed
    out['clusters'] = int(counts.sum().item())

    # the same four layers as float64 matmuls on the same F
    F = []
    for r in rooms:
        nb = baselines_ref.neighbours(r['points'], 0.1)
        mn, mx = edge_ref.bounds(r['points'], nb)
        ii, ss = np.nonzero(nb[:, 13:] >= 0)
        kk = nb[ii, 13 + ss]
        F.append(edge_ref.edge_rows(r['points'][ii], r['points'][kk], mn[ii], mn[kk], mx[ii], mx[kk]))
    Fd = torch.from_numpy(np.concatenate(F).astype(np.float64)).to(dev)
    assert len(Fd) == edges
    Wd = [torch.from_numpy(w).to(dev) for w in weights]

    def run_torch():
        h = Fd
        for l in range(4):
            h = torch.addmm(Wd[2 * l + 1], h, Wd[2 * l])
            if l < 3:
                h = torch.relu_(h)
        return h
    out['torch_float64_matmul_s'] = timed(torch, run_torch, args.min_seconds)
    zt = run_torch()[:, 0].cpu().numpy()
    out['torch_largest_logit_difference'] = float(np.abs(zt - zh[~np.isnan(zh)]).max())       # same slots in the same (row-major) order
    out['logits_over_torch'] = out['logits_s'] / out['torch_float64_matmul_s']

    # edges within 1e-9 of a threshold (host route)
    near = 0
    ph = expit(zh)
    for r in range(R):
        s, e = int(room_start[r]), int(room_start[r + 1])
        nb = baselines_ref.neighbours(rooms[r]['points'], 0.1)
        pmax, _ = edge_ref.keep_words(ph[s:e], nb)
        ii, ss = np.nonzero(nb[:, 13:] >= 0)
        q = ph[s:e][ii, ss]
        kk = nb[ii, 13 + ss]
        gap = np.minimum(np.minimum(np.abs(q - 0.99 * pmax[ii]), np.abs(q - 0.99 * pmax[kk])), np.abs(q - 0.9))
        near += int((gap <= 1e-9).sum())
    out['edges_within_1e-9_of_a_threshold'] = near
    out['share_within_1e-9'] = near / max(1, edges)

    for route in ('host', 'device'):
        edge.segment(rooms, model, sigmoid=route)
        torch.cuda.synchronize()
        t0, k = time.time(), 0
        while time.time() - t0 < args.min_seconds:
            edge.segment(rooms, model, sigmoid=route)
            k += 1
        torch.cuda.synchronize()
        out['rooms_per_s_' + route] = R * k / (time.time() - t0)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == '__main__':
    main()
