#!/usr/bin/env python3
"""Measure the FPFH mode (learn_region_grow_amd.baselines: fpfh, segment(..., 'fpfh')) -> profiles/fpfh_bench.json.

The 68 Area-5-shaped rooms (synthetic.area5_shaped_room at AREA5_POINTS, 0.1 m, the raw rooms workloads.area5_rooms preprocesses),
rooms/s of each stage end to end (HIP events around the stage, warm, repeated for at least --min-seconds):
  features     room_features for every room (device equalisation and covariances, host numpy.linalg.svd)
  descriptor   baselines.fpfh: the PCD round trip on the host, the upload, ONE lrg_fpfh call, the download
  segment      segment(rooms carrying 'fpfh', 'fpfh'): ONE lrg_baseline_segment_fpfh call
and, for scale, segment(..., 'normal') on the same rooms.  lrg_fpfh alone (inputs resident, 10 calls between two events) with the
gather pass probing the window again and with stored neighbour lists (LRG_FPFH_LISTS).  The two passes' own kernel times come from
separate `rocprofv3 --kernel-trace --stats` runs of `--only-device probe` and `--only-device lists` (--kernel-stats, --kernel-stats-lists).
Nothing is asserted.

    python tools/fpfh_bench.py [--out profiles/fpfh_bench.json] [--kernel-stats probe_kernel_stats.csv] [--kernel-stats-lists lists_kernel_stats.csv]
"""
import argparse
import csv
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def timed(torch, fn, min_seconds):
    """fn() once to warm up, then repeated for at least min_seconds: (seconds per call by HIP events, the last result)."""
    res = fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps, total = 0, 0.0
    while total < min_seconds:
        e0.record()
        res = fn()
        e1.record()
        e1.synchronize()
        total += e0.elapsed_time(e1) / 1e3
        reps += 1
    return (total / reps if reps else 0.0), res


def device_time(B, lib, torch, feats, flags, min_seconds):
    """lrg_fpfh alone: inputs on the device, 10 calls between two events."""
    dev = torch.device('cuda:0')
    starts = np.concatenate([[0], np.cumsum([len(f['points']) for f in feats])]).astype(np.int32)
    n = int(starts[-1])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    pts = up(np.concatenate([f['points'][:, :3] for f in feats]))
    xyz = up(np.concatenate([B.pcd_roundtrip(f['points'][:, :3]) for f in feats]))
    nrm = up(np.concatenate([B.pcd_roundtrip(f['normals'].astype(np.float32)) for f in feats]))
    ws = torch.empty(lib.lrg_fpfh_workspace_bytes(n, len(feats), flags), dtype=torch.uint8, device=dev)
    counts = torch.empty((n, 33), dtype=torch.int32, device=dev)
    k = torch.empty(n, dtype=torch.int32, device=dev)
    out = torch.empty((n, 33), dtype=torch.float32, device=dev)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def ten():
        for _ in range(10):
            rc = lib.lrg_fpfh(p(pts), 3, p(xyz), p(nrm), starts.ctypes.data_as(ctypes.c_void_p), len(feats), ctypes.c_float(0.1), ctypes.c_float(0.2),
                              flags, p(ws), ws.numel(), p(counts), p(k), p(out), st)
            assert rc == 0, rc
    s, _ = timed(torch, ten, min_seconds)
    return dict(device_s=s / 10, points_per_s=n / (s / 10), mean_neighbours=float(k.float().mean().item()) - 1.0, max_k=int(k.max().item()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'fpfh_bench.json'))
    ap.add_argument('--min-seconds', type=float, default=0.5)
    ap.add_argument('--rooms', type=int, default=68)
    ap.add_argument('--kernel-stats', default=None, help='kernel_stats.csv of a rocprofv3 run of --only-device probe')
    ap.add_argument('--kernel-stats-lists', default=None, help='kernel_stats.csv of a rocprofv3 run of --only-device lists')
    ap.add_argument('--only-device', default=None, choices=('probe', 'lists'), help='lrg_fpfh alone in one gather form, nothing written (the rocprofv3 runs)')
    args = ap.parse_args()
    import torch
    from learn_region_grow_amd import _lib, baselines as B, synthetic
    lib = _lib.load()
    raws = [synthetic.area5_shaped_room(t, 1000 + i).astype(np.float32) for i, t in enumerate(synthetic.AREA5_POINTS[:args.rooms])]
    f_s, feats = timed(torch, lambda: [B.room_features(r) for r in raws], 0.0 if args.only_device else args.min_seconds)
    n = sum(len(f['points']) for f in feats)
    if args.only_device:
        print('lrg_fpfh', args.only_device, json.dumps(device_time(B, lib, torch, feats, _lib.LRG_FPFH_LISTS if args.only_device == 'lists' else 0, args.min_seconds)))
        return
    probe = device_time(B, lib, torch, feats, 0, args.min_seconds)
    lists = device_time(B, lib, torch, feats, _lib.LRG_FPFH_LISTS, args.min_seconds)
    print('lrg_fpfh', json.dumps(dict(probe=probe, lists=lists)))
    d_s, hist = timed(torch, lambda: B.fpfh(feats), args.min_seconds)
    rooms = [dict(f, fpfh=h) for f, h in zip(feats, hist)]
    s_s, labels = timed(torch, lambda: B.segment(rooms, 'fpfh'), args.min_seconds)
    n_s, _ = timed(torch, lambda: B.segment(feats, 'normal'), args.min_seconds)
    out = dict(device=torch.cuda.get_device_name(0), measured_on='MI355X (gfx950)', rooms=len(raws), equalized_points=n,
               clusters=int(sum(int(l.max()) for l in labels)),
               stages=dict(features=dict(seconds=f_s, rooms_per_s=len(raws) / f_s), descriptor=dict(seconds=d_s, rooms_per_s=len(raws) / d_s),
                           segment=dict(seconds=s_s, rooms_per_s=len(raws) / s_s),
                           all=dict(seconds=f_s + d_s + s_s, rooms_per_s=len(raws) / (f_s + d_s + s_s))),
               segment_normal=dict(seconds=n_s, rooms_per_s=len(raws) / n_s),
               lrg_fpfh=dict(gather_probes_again=probe, gather_reads_lists=lists),
               notes=['stages: HIP events around each stage end to end (host work, copies and kernels), one warm-up call, then >= min-seconds of repeats',
                      'lrg_fpfh: the C call alone, inputs resident, 10 calls between two events'])
    for key, path in (('kernel_stats_probe', args.kernel_stats), ('kernel_stats_lists', args.kernel_stats_lists)):
        if path and os.path.exists(path):
            out[key] = {row['Name']: dict(calls=int(row['Calls']), avg_ns=float(row['AverageNs']), total_ns=float(row['TotalDurationNs']))
                        for row in csv.DictReader(open(path)) if row['Name'].startswith('fp_')}
            out['notes'].append(key + ': rocprofv3 --kernel-trace --stats of `--only-device ' + key.split('_')[-1] + '`')
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out['stages']), json.dumps(out['segment_normal']))
    print('wrote', args.out)


if __name__ == '__main__':
    main()
