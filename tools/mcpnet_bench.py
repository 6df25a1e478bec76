#!/usr/bin/env python3
"""Measure MCPNet on the GPU (learn_region_grow_amd.mcpnet) -> profiles/mcpnet_bench.json.

Sets: the 68 Area-5-shaped rooms (synthetic.area5_shaped_room at AREA5_POINTS, centred and equalised at 0.1 m) in one batch, and one
100 k-point KITTI-shaped scene.  Device times by HIP events (warm-up, then repeats for at least --min-seconds): lrg_mcp_embed and its
fraction of the 157.3 TFLOP/s fp32 matrix peak at 4.2056 MFLOP per point (2 102 800 MAC), the candidate build plus counter draws,
the segmentation; host time of the legacy draws; end-to-end rooms/s in both RNG modes (room preparation included); the NumPy
restatement's seconds per room as the CPU figure.  Per-kernel medians come from a separate `rocprofv3 --kernel-trace --stats` run of
`--only-device` (pass its kernel_stats.csv with --kernel-stats to fold them in).

    python tools/mcpnet_bench.py [--out profiles/mcpnet_bench.json] [--weights tests/golden/mcpnet_model5_weights.npz]
"""
import argparse
import csv
import ctypes
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

PEAK_TFLOPS = 157.3
MAC_PER_POINT = 50 * (6 * 200 + 200 * 200) + 204 * 200 + 200 * 10        # 2 102 800


def timed(torch, fn, min_seconds, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    t_end = time.time() + min_seconds
    while time.time() < t_end or len(times) < 5:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    return float(np.median(times)), len(times)


def measure_set(name, raws, net, weights, args, torch):
    from learn_region_grow_amd import _lib, mcpnet
    lib = _lib.load()
    dev = torch.device('cuda:0')
    t0 = time.time()
    rooms = [mcpnet.prepare_room(r, room_id=k) for k, r in enumerate(raws)]
    prep = time.time() - t0
    room_start, n, pts = mcpnet._batch(rooms, dev)
    rs_p = room_start.ctypes.data_as(ctypes.c_void_p)
    ws = torch.empty(lib.lrg_mcp_workspace_bytes(n, len(rooms)), dtype=torch.uint8, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    nbr = torch.empty((n, 50), dtype=torch.int32, device=dev)
    ids = np.arange(len(rooms), dtype=np.int32)
    st = mcpnet._stream

    def cand_counter():
        _lib.check(lib.lrg_mcp_candidates(mcpnet._ptr(pts), 6, rs_p, len(rooms), mcpnet._ptr(ws), ws.numel(), mcpnet._ptr(counts), st()), 'cand')
        _lib.check(lib.lrg_mcp_neighbors(mcpnet._ptr(pts), 6, rs_p, len(rooms), mcpnet._ptr(ws), ws.numel(), None, 0,
                                         ids.ctypes.data_as(ctypes.c_void_p), mcpnet._ptr(nbr), st()), 'nbr')
    t_cand, k_cand = timed(torch, cand_counter, args.min_seconds)
    out = torch.empty((n, 10), dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    t_emb, k_emb = timed(torch, lambda: net.embed_device(pts, nbr, out=out, status=status), args.min_seconds)
    assert int(status.item()) == 0
    emb = out.cpu().numpy()
    starts = room_start.astype(np.int64)
    embs = [emb[starts[r]:starts[r + 1]] for r in range(len(rooms))]
    emb_t = torch.from_numpy(emb).to(dev)
    wsb = torch.empty(lib.lrg_baseline_workspace_bytes(n, len(rooms), 10), dtype=torch.uint8, device=dev)
    lab = torch.empty(n, dtype=torch.int32, device=dev)
    cnt = torch.empty(len(rooms), dtype=torch.int32, device=dev)
    t_seg, k_seg = timed(torch, lambda: _lib.check(lib.lrg_baseline_segment_embedding(
        mcpnet._ptr(pts), 6, rs_p, len(rooms), ctypes.c_float(0.1), mcpnet._ptr(emb_t), 10, 0.9, 10, mcpnet._ptr(wsb), wsb.numel(),
        mcpnet._ptr(lab), mcpnet._ptr(cnt), st()), 'seg'), args.min_seconds)
    cnt_h = counts.cpu().numpy()
    t0 = time.time()
    mcpnet.legacy_positions(cnt_h, np.random.RandomState(0))
    t_legacy = time.time() - t0
    e2e = {}
    for rng in ('counter', 'legacy'):
        torch.cuda.synchronize()
        t0 = time.time()
        rr = [mcpnet.prepare_room(r, room_id=k) for k, r in enumerate(raws)]
        nb = mcpnet.neighbors(rr, rng=rng, seed=0)
        ee = net.embed([r['points'] for r in rr], nb)
        mcpnet.segment(rr, ee)
        e2e[rng] = len(raws) / (time.time() - t0)
    flop = 2.0 * MAC_PER_POINT * n
    res = dict(set=name, rooms=len(rooms), points=n, prepare_s=prep,
               embed_s=t_emb, embed_repeats=k_emb, embed_tflops=flop / t_emb * 1e-12, embed_fraction_of_peak=flop / t_emb * 1e-12 / PEAK_TFLOPS,
               floor_at_peak_s=flop / (PEAK_TFLOPS * 1e12),
               candidates_counter_s=t_cand, candidates_counter_repeats=k_cand, segment_s=t_seg, segment_repeats=k_seg,
               legacy_host_draw_s=t_legacy, rooms_per_s_counter=e2e['counter'], rooms_per_s_legacy=e2e['legacy'])
    print(json.dumps(res))
    return res, rooms, embs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'mcpnet_bench.json'))
    ap.add_argument('--weights', default=os.path.join(REPO, 'tests', 'golden', 'mcpnet_model5_weights.npz'))
    ap.add_argument('--min-seconds', type=float, default=0.5)
    ap.add_argument('--only-device', action='store_true', help='the Area-5 set only, no CPU figure (for the rocprofv3 run)')
    ap.add_argument('--kernel-stats', default=None)
    args = ap.parse_args()
    import torch
    from learn_region_grow_amd import mcpnet, synthetic
    z = np.load(args.weights)
    weights = {k: z[k] for k in z.files}
    net = mcpnet.MCPNetHIP(weights)
    area5 = [synthetic.area5_shaped_room(t, 1000 + i).astype(np.float32) for i, t in enumerate(synthetic.AREA5_POINTS[:68])]
    out = dict(device=torch.cuda.get_device_name(0), peak_tflops=PEAK_TFLOPS, mac_per_point=MAC_PER_POINT, sets=[])
    r5, rooms5, embs5 = measure_set('area5_68_rooms', area5, net, weights, args, torch)
    out['sets'].append(r5)
    if not args.only_device:
        kitti = [synthetic.area5_shaped_room(100000, 5000, resolution=0.3).astype(np.float32)]
        out['sets'].append(measure_set('kitti_100k_scene', kitti, net, weights, args, torch)[0])
        import mcpnet_ref as R
        t0 = time.time()
        for k in range(2):
            p = rooms5[k]['points']
            nb = R.legacy_neighbors(R.candidates(p), np.random.RandomState(0))
            R.forward(weights, p, nb, dtype=np.float32)
            R.components(p, embs5[k])
        out['cpu_restatement_s_per_room'] = (time.time() - t0) / 2
        out['cpu_restatement_rooms'] = [len(rooms5[k]['points']) for k in range(2)]
    if args.kernel_stats and os.path.exists(args.kernel_stats):
        with open(args.kernel_stats) as f:
            out['kernel_stats'] = [{k: row[k] for k in row if k in ('Name', 'Calls', 'TotalDurationNs', 'AverageNs', 'Percentage', 'MinNs', 'MaxNs')}
                                   for row in csv.DictReader(f)][:30]
    if not args.only_device:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
        print('wrote', args.out)


if __name__ == '__main__':
    main()
