#!/usr/bin/env python3
"""Measure the benchmarks.py baselines on the GPU (learn_region_grow_amd.baselines) -> profiles/baselines_bench.json.

Per mode: the 68 Area-5-shaped rooms (synthetic.area5_shaped_room at AREA5_POINTS, 0.1 m) in ONE lrg_baseline_segment call, and
one 100 k-point KITTI-shaped scene (area5_shaped_room(100000, seed, resolution=0.3), as workloads.kitti_scenes builds it) at
0.3 m.  Device time of the segmentation by HIP events (warm-up, then repeats for at least --min-seconds), end-to-end rooms/s
including room_features (device equalisation and covariances, host SVD) and the host SVD's share, and the CPU restatement
(tests/baselines_ref.py) on a few rooms.  Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of
`--only-device` (pass its kernel_stats.csv with --kernel-stats to fold them in).

    python tools/baselines_bench.py [--out profiles/baselines_bench.json] [--kernel-stats kernel_stats.csv]
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

L2_TBS = 34.5          # MI355X aggregate L2 bandwidth (measured figure of the microarchitecture notes)
HBM_TBS = 6.3          # achievable HBM bandwidth (8 TB/s peak)


def make_sets(resolution_kitti=0.3):
    from learn_region_grow_amd import synthetic
    area5 = [synthetic.area5_shaped_room(t, 1000 + i).astype(np.float32) for i, t in enumerate(synthetic.AREA5_POINTS[:68])]
    kitti = [synthetic.area5_shaped_room(100000, 5000, resolution=resolution_kitti).astype(np.float32)]
    return area5, kitti


def device_time(B, lib, torch, rooms, mode, resolution, min_seconds):
    """Events around lrg_baseline_segment alone (inputs already on the device)."""
    dev = torch.device('cuda:0')
    t = B.default_thresholds(mode)
    sizes = [len(r['points']) for r in rooms]
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(starts[-1])
    pts = torch.from_numpy(np.concatenate([r['points'] for r in rooms])).to(dev)
    nrm = torch.from_numpy(np.concatenate([r['normals'] for r in rooms])).to(dev) if mode != 'color' else None
    cur = torch.from_numpy(np.concatenate([r['curvatures'] for r in rooms])).to(dev) if mode != 'color' else None
    rnk = torch.from_numpy(np.concatenate([r['rank'] for r in rooms])).to(dev) if mode != 'color' else None
    ws = torch.empty(lib.lrg_baseline_workspace_bytes(n, len(rooms), 10), dtype=torch.uint8, device=dev)
    lab = torch.empty(n, dtype=torch.int32, device=dev)
    cnt = torch.empty(len(rooms), dtype=torch.int32, device=dev)
    p = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def once():
        rc = lib.lrg_baseline_segment(p(pts), 6, starts.ctypes.data_as(ctypes.c_void_p), len(rooms), ctypes.c_float(resolution),
                                      B.MODES.index(mode), p(nrm), p(cur), p(rnk), t[0], t[1], t[2], 10, p(ws), ws.numel(), p(lab), p(cnt), st)
        assert rc == 0, rc
    for _ in range(3):
        once()
    torch.cuda.synchronize()
    reps, total = 0, 0.0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    while total < min_seconds:
        k = max(1, reps)
        e0.record()
        for _ in range(k):
            once()
        e1.record()
        e1.synchronize()
        total += e0.elapsed_time(e1) / 1e3
        reps += k
    return total / reps, n, int(cnt.sum().item())


def union_bytes(rooms, resolution):
    """Bytes the edge-and-union pass must move at least, per the access pattern: per point its xyz (12 B), 26 probes of a 12-B
    hash slot, and per neighbour found its features (normals 24 B, curvature 8 B, rgb 12 B) and two parent words (8 B)."""
    import baselines_ref as R
    found = sum(int((R.neighbours(r['points'], resolution) >= 0).sum()) for r in rooms)
    n = sum(len(r['points']) for r in rooms)
    return n * (12 + 26 * 12 + 24 + 8 + 12) + found * (24 + 8 + 12 + 8), found / max(n, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'baselines_bench.json'))
    ap.add_argument('--min-seconds', type=float, default=0.5)
    ap.add_argument('--kernel-stats', default=None)
    ap.add_argument('--only-device', action='store_true', help='device timing only (the rocprofv3 run)')
    args = ap.parse_args()
    import torch
    from learn_region_grow_amd import _lib, baselines as B
    import baselines_ref as R
    lib = _lib.load()
    area5_raw, kitti_raw = make_sets()
    out = dict(device=torch.cuda.get_device_name(0), measured_on='MI355X (gfx950)', modes={},
               notes=['device_s: HIP events around lrg_baseline_segment alone, inputs resident, after 3 warm-up calls',
                      'end_to_end: room_features for every room (device equalisation + covariances, host numpy.linalg.svd) + one segment call, wall clock',
                      'reference benchmarks.py itself: ~3 s per 15 k-equalised-point room per mode, measured on the build machine CPU (not on the GPU machine)'])
    sets = {}
    for name, raws, res in (('area5_68', area5_raw, 0.1), ('kitti_100k', kitti_raw, 0.3)):
        t0 = time.time()
        feats = [B.room_features(r, resolution=res) for r in raws]
        t_feat = time.time() - t0
        t0 = time.time()
        for r in raws:
            B.room_features(r, resolution=res, need_normals=False)
        t_eq = time.time() - t0
        sets[name] = (feats, res, t_feat, t_eq)
    for mode in B.MODES:
        md = {}
        for name, (feats, res, t_feat, t_eq) in sets.items():
            dt, n, ncl = device_time(B, lib, torch, feats, mode, res, args.min_seconds)
            d = dict(rooms=len(feats), equalized_points=n, clusters=ncl, device_s=dt, points_per_s=n / dt, rooms_per_s=len(feats) / dt)
            if not args.only_device:
                t0 = time.time()
                B.segment(feats, mode, resolution=res)
                seg_wall = time.time() - t0
                ft = t_eq if mode == 'color' else t_feat
                d.update(features_s=ft, segment_wall_s=seg_wall, end_to_end_rooms_per_s=len(feats) / (ft + seg_wall),
                         host_svd_share=0.0 if mode == 'color' else (t_feat - t_eq) / (ft + seg_wall))
            md[name] = d
        if not args.only_device:
            few = sets['area5_68'][0][:3]
            t0 = time.time()
            for f in few:
                R.segment(f, mode, B.default_thresholds(mode))
            md['cpu_restatement_s_per_room'] = (time.time() - t0) / len(few)
            md['cpu_restatement_rooms'] = [len(f['points']) for f in few]
        out['modes'][mode] = md
        print(mode, json.dumps({k: {kk: (round(vv, 6) if isinstance(vv, float) else vv) for kk, vv in v.items()} if isinstance(v, dict) else v
                                for k, v in md.items()}))
    if args.only_device:
        return
    nbytes, nb_per_pt = union_bytes(sets['area5_68'][0], 0.1)
    out['union_pass'] = dict(bytes_floor_area5=nbytes, neighbours_per_point=nb_per_pt)
    if args.kernel_stats and os.path.exists(args.kernel_stats):
        ks = {}
        for row in csv.DictReader(open(args.kernel_stats)):
            ks[row['Name']] = dict(calls=int(row['Calls']), avg_ns=float(row['AverageNs']), total_ns=float(row['TotalDurationNs']))
        out['kernel_stats'] = ks
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
