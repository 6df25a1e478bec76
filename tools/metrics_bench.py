#!/usr/bin/env python3
"""Measure the evaluation block on the host and on the device -> profiles/metrics_bench.json.

Two sets: the 68 Area-5-shaped rooms of bench.py (workloads.area5_rooms, 0.1 m) and the eight 100 k-point KITTI-shaped scenes
(workloads.kitti_scenes, 0.3 m), each grown once with the configuration of the benchmark's steady leg (trained weights, the network's
policy, the counter stream, one restart) and filled in.  Per set:

  host     metrics.room_metrics room by room (NumPy + sklearn), repeated; and with_sklearn=False, whose difference is sklearn's share
  device   metrics_gpu.room_metrics_batch: lrg_metrics_batch alone between two events (inputs resident, after warm-up, >= 5 repeats:
           median and minimum), and the whole path by the wall clock -- ground-truth preparation, uploads, the call, the copies back and
           the host finish -- with its parts; the EMI term count of every room
  check    the device's dicts against the host's: prc / rcl / iou / cluster_label2 / ars equal, the largest |nmi| and |ami| difference

The verdict per set: the whole device path (its slowest repeat) against the host block (its fastest repeat).

    python tools/metrics_bench.py [--out profiles/metrics_bench.json] [--repeats 5] [--host-repeats 3] [--cache DIR]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def grow(torch, rooms, resolution, dev):
    from learn_region_grow_amd import synthetic
    from learn_region_grow_amd.grow import RegionGrower
    from learn_region_grow_amd.lrgnet import LrgNetHIP
    net = LrgNetHIP(1, 1, 512, 512, 13, 0, device=dev).load_weights(synthetic.load_trained_weights())
    t0 = time.perf_counter()
    results = RegionGrower(net, rooms_in_flight=len(rooms), restarts=1, rng='counter', seed=0, policy='net', resolution=resolution).run(rooms)
    torch.cuda.synchronize()
    return [np.asarray(r.filled_label).astype(np.int64) for r in results], time.perf_counter() - t0


def spread(xs):
    xs = sorted(xs)
    return dict(median=float(np.median(xs)), min=float(xs[0]), max=float(xs[-1]), repeats=len(xs))


def measure(torch, name, rooms, labels, dev, repeats, host_repeats):
    from learn_region_grow_amd import metrics, metrics_gpu
    objs = [np.asarray(r['obj_id']) for r in rooms]
    R = len(rooms)
    # ---- host ----
    host_full, host_plain, want = [], [], None
    for _ in range(host_repeats):
        t0 = time.perf_counter()
        want = [metrics.room_metrics(o, l) for o, l in zip(objs, labels)]
        host_full.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        for o, l in zip(objs, labels):
            metrics.room_metrics(o, l, with_sklearn=False)
        host_plain.append(time.perf_counter() - t0)
    # ---- device: the whole path ----
    metrics_gpu.room_metrics_batch(objs, labels, device=dev)                     # warm-up (code objects, allocator)
    path, parts, got = [], [], None
    for _ in range(repeats):
        timing = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = metrics_gpu.room_metrics_batch(objs, labels, device=dev, timing=timing)
        path.append(time.perf_counter() - t0)
        parts.append(timing)
    # ---- device: the call alone, inputs resident ----
    prep = [metrics_gpu.prepare_ground_truth(o) for o in objs]
    dev_labels = [torch.from_numpy(l.astype(np.int32)).to(dev) for l in labels]
    ncl = [int(l.max()) for l in labels]
    call, raw = [], None
    for _ in range(repeats + 1):
        timing = {}
        raw = metrics_gpu.run_batch(prep, dev_labels, device=dev, n_clusters=ncl, timing=timing)
        call.append(timing['device_events'])
    call = call[1:]
    # ---- agreement ----
    d_nmi = d_ami = 0.0
    equal = True
    for g, w in zip(got, want):
        equal &= all(g[k] == w[k] or (np.isnan(g[k]) and np.isnan(w[k])) for k in ('prc', 'rcl', 'iou', 'ars'))
        equal &= bool(np.array_equal(g['cluster_label2'], w['cluster_label2']))
        d_nmi, d_ami = max(d_nmi, abs(g['nmi'] - w['nmi'])), max(d_ami, abs(g['ami'] - w['ami']))
    lines_equal = all(metrics.room_line(5, k, g) == metrics.room_line(5, k, w) for k, (g, w) in enumerate(zip(got, want)))
    terms = [int(v) for v in raw['int_sums'][:, 6]]
    h, p = spread(host_full), spread(path)
    out = dict(rooms=R, points=int(sum(len(o) for o in objs)), gt_instances=[int(len(np.unique(o))) for o in objs], clusters=ncl,
               emi_terms_per_room=terms, emi_terms=int(sum(terms)),
               host_seconds=h, host_without_sklearn_seconds=spread(host_plain),
               host_sklearn_share=1.0 - float(np.median(host_plain)) / h['median'], host_rooms_per_s=R / h['median'],
               device_call_seconds=spread(call), device_path_seconds=p, device_path_rooms_per_s=R / p['median'],
               device_path_parts_seconds={k: spread([t.get(k, 0.0) for t in parts]) for k in ('prepare', 'uploads', 'device', 'downloads', 'finish')},
               speedup_median=h['median'] / p['median'],
               device_beats_host_beyond_spread=bool(p['max'] < h['min']),
               matching_outputs_and_ars_equal=bool(equal), room_lines_equal=bool(lines_equal), max_abs_nmi_diff=d_nmi, max_abs_ami_diff=d_ami)
    print('%s: host %.3f s (%.1f rooms/s, sklearn %.0f %%), device path %.4f s (%.0f rooms/s; call alone %.4f s), x%.1f; nmi %.1e ami %.1e equal %s'
          % (name, h['median'], out['host_rooms_per_s'], 100 * out['host_sklearn_share'], p['median'], out['device_path_rooms_per_s'],
             out['device_call_seconds']['median'], out['speedup_median'], d_nmi, d_ami, equal and lines_equal))
    sys.stdout.flush()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'metrics_bench.json'))
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--host-repeats', type=int, default=3)
    ap.add_argument('--cache', default=os.environ.get('LRG_CACHE'))
    ap.add_argument('--sets', default='area5,kitti')
    args = ap.parse_args()
    import torch
    from learn_region_grow_amd import workloads
    if not torch.cuda.is_available():
        raise SystemExit('metrics_bench.py needs a GPU: a host run measures nothing of the device path')
    if args.repeats < 5:
        raise SystemExit('--repeats: at least five')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    out = dict(device=torch.cuda.get_device_name(0), sklearn=__import__('sklearn').__version__, sets={})
    for name in args.sets.split(','):
        if name == 'area5':
            rooms, res = workloads.area5_rooms(68, seed_base=1000, cache_dir=args.cache), 0.1
        else:
            rooms, res = workloads.kitti_scenes(8, seed_base=5000, cache_dir=args.cache), 0.3
        labels, t_grow = grow(torch, rooms, res, dev)
        m = measure(torch, name, rooms, labels, dev, args.repeats, args.host_repeats)
        m['grow_seconds_once_cold'] = t_grow
        out['sets'][name] = m
        with open(args.out, 'w') as f:                    # (after every set: a later set that runs out of time keeps the earlier one)
            json.dump(out, f, indent=1)
            f.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
