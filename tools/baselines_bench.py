#!/usr/bin/env python3
"""Measure the benchmarks.py baselines on the GPU (learn_region_grow_amd.baselines) -> profiles/baselines_bench.json.

Per mode: the 68 Area-5-shaped rooms (synthetic.area5_shaped_room at AREA5_POINTS, 0.1 m) in ONE lrg_baseline_segment call, and
one 100 k-point KITTI-shaped scene (area5_shaped_room(100000, seed, resolution=0.3), as workloads.kitti_scenes builds it) at
0.3 m.  Device time of the segmentation by HIP events (warm-up, then repeats for at least --min-seconds), end-to-end rooms/s
including room_features (device equalisation and covariances, host SVD) and the host SVD's share, and the CPU restatement
(tests/baselines_ref.py) on a few rooms.  Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of
`--only-device` (pass its kernel_stats.csv with --kernel-stats to fold them in).

Both feature routes end to end ("routes" in the output): room_features(eig='lapack' | 'verified') for every room and one segment call per
mode that reads normals, events around the whole pass, warm, repeated for at least --min-seconds; the device times of lrg_baseline_eig
(all rooms' covariances in one call) and lrg_baseline_certify alone; the shares of points the verified route sends through LAPACK; and
where its remaining time goes (the per-room lrg_preprocess calls, the host argsorts).

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


def timed(torch, fn, min_seconds):
    """fn() once to warm up, then repeated for at least min_seconds between two events: (seconds per call by the events, by the wall
    clock, the last result)."""
    res = fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps, total, wall = 0, 0.0, 0.0
    while total < min_seconds:
        t0 = time.time()
        e0.record()
        res = fn()
        e1.record()
        e1.synchronize()
        wall += time.time() - t0
        total += e0.elapsed_time(e1) / 1e3
        reps += 1
    return total / reps, wall / reps, res


def routes(B, lib, torch, raws, res, min_seconds):
    """The 'lapack' and the 'verified' feature route end to end on one set, per mode that reads normals."""
    dev = torch.device('cuda:0')
    p = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None
    modes = [m for m in B.MODES if m != 'color']
    out = dict(rooms=len(raws), modes={})

    def run(route, mode):
        feats = [B.room_features(r, resolution=res, eig=route) for r in raws]
        labels, stats = B.segment(feats, mode, resolution=res, return_stats=True)
        return feats, labels, stats
    for mode in modes:
        md = {}
        keep = {}
        for route in ('lapack', 'verified'):
            ev, wall, (feats, labels, stats) = timed(torch, lambda: run(route, mode), min_seconds)
            keep[route] = labels
            md[route] = dict(end_to_end_s=ev, end_to_end_wall_s=wall, rooms_per_s=len(raws) / ev)
            if route == 'verified':
                n = sum(len(f['points']) for f in feats)
                md[route].update(certificate_flagged_share=float(sum(stats['flagged'])) / n,
                                 certificate_flagged_share_worst_room=max(float(k) / len(f['points']) for k, f in zip(stats['flagged'], feats)))
        md['labels_equal'] = all(np.array_equal(a, b) for a, b in zip(keep['lapack'], keep['verified']))
        md['verified_over_lapack'] = md['lapack']['end_to_end_s'] / md['verified']['end_to_end_s']
        out['modes'][mode] = md
    # the verified route's parts, each alone
    ev_f, wall_f, feats = timed(torch, lambda: [B.room_features(r, resolution=res, eig='verified') for r in raws], min_seconds)
    ev_l, _, _ = timed(torch, lambda: [B.room_features(r, resolution=res) for r in raws], min_seconds)
    ev_p, _, _ = timed(torch, lambda: [B.room_features(r, resolution=res, need_normals=False) for r in raws], min_seconds)
    n = sum(len(f['points']) for f in feats)
    curv = [f['curvatures'] for f in feats]
    t0, reps = time.time(), 0
    while time.time() - t0 < min_seconds:
        for c in curv:                                          # room_features sorts twice: to find the close pairs, then for the rank
            np.argsort(c)
            np.argsort(c)
        reps += 1
    argsort_s = (time.time() - t0) / reps
    cov = torch.from_numpy(np.concatenate([f['cov'] for f in feats])).to(dev)
    nrm = torch.empty((n, 3), dtype=torch.float64, device=dev)
    sol = torch.empty((3, n), dtype=torch.float64, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def eig_once():
        assert lib.lrg_baseline_eig(p(cov), n, p(nrm), p(sol[0]), p(sol[1]), p(sol[2]), st) == 0
    eig_s, _, _ = timed(torch, lambda: [eig_once() for _ in range(20)], min_seconds)
    starts = np.concatenate([[0], np.cumsum([len(f['points']) for f in feats])]).astype(np.int32)
    pts = torch.from_numpy(np.concatenate([f['points'] for f in feats])).to(dev)
    cur = sol[0].contiguous()
    ws = torch.empty(lib.lrg_baseline_workspace_bytes(n, len(feats), 10), dtype=torch.uint8, device=dev)
    flags = torch.empty(n, dtype=torch.int32, device=dev)
    nfl = torch.empty(1, dtype=torch.int32, device=dev)
    cert = {}
    for mode in modes:
        t = B.default_thresholds(mode)

        def cert_once():
            assert lib.lrg_baseline_certify(p(pts), 6, starts.ctypes.data_as(ctypes.c_void_p), len(feats), ctypes.c_float(res), B.MODES.index(mode),
                                            p(nrm), p(cur), p(sol[1]), p(sol[2]), t[0], t[1], t[2], 10, p(ws), ws.numel(), p(flags), p(nfl), st) == 0
        cert[mode] = timed(torch, lambda: [cert_once() for _ in range(20)], min_seconds)[0] / 20
    redone = sum(f['verify_stats']['rank_redone'] for f in feats)
    degenerate = sum(f['verify_stats']['degenerate'] for f in feats)
    out.update(equalized_points=n, features_verified_s=ev_f, features_verified_wall_s=wall_f, features_lapack_s=ev_l,
               preprocess_calls_s=ev_p, preprocess_calls_share_of_verified_features=ev_p / ev_f,
               host_argsort_s=argsort_s, host_argsort_share_of_verified_features=argsort_s / ev_f,
               lrg_baseline_eig_device_s=eig_s / 20, lrg_baseline_eig_points_per_s=n / (eig_s / 20), lrg_baseline_certify_device_s=cert,
               rank_redone_share=redone / n, rank_redone_share_worst_room=max(f['verify_stats']['rank_redone'] / f['verify_stats']['points'] for f in feats),
               degenerate_share=degenerate / n)
    return out


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
    ap.add_argument('--only-routes', action='store_true', help="only the comparison of the 'lapack' and 'verified' feature routes (printed, not written)")
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
    if not args.only_device:
        out['routes'] = {}
        for name, raws, res in (('area5_68', area5_raw, 0.1), ('kitti_100k', kitti_raw, 0.3)):
            out['routes'][name] = routes(B, lib, torch, raws, res, args.min_seconds)
            print('routes', name, json.dumps(out['routes'][name]))
        out['notes'].append("routes: room_features(eig=...) for every room + one segment call, events around the pass, warm, >= min-seconds of repeats; "
                            "preprocess_calls_s = the same loop with need_normals=False (the per-room lrg_preprocess calls and their copies); "
                            "host_argsort_s = two numpy.argsort per room; kernel times: 20 calls between two events")
        if args.only_routes:
            return
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
