#!/usr/bin/env python
"""Staging the 68 Area-5-shaped rooms of learn_region_grow_amd.workloads: the host path (stage.stage_room, legacy draws, one room after
the other, then center_tuples) against the device teacher (stage.stage_rooms_gpu, counter draws: upload, lrg_stage_teacher,
lrg_stage_tuples, download) on the same commit and machine.  Writes profiles/stage_bench.json.

The two paths draw from different streams, so they stage different (equally distributed) tuples: the comparison is of the time per
room set and per tuple, not of the bytes.  Wall times are host clocks around work that ends synchronised (stage_rooms_gpu returns NumPy
arrays); kernel times are device events around each launch.  The device path is warmed (first launches load the code object) and
repeated; every repeat is listed, with median and range.

    python tools/stage_bench.py [--rooms 68] [--repeats 5] [--host-repeats 2] [--out profiles/stage_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def spread(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)), runs=[float(x) for x in xs])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--rooms', type=int, default=68)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--host-repeats', type=int, default=2)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--cache-dir', default=None)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'stage_bench.json'))
    args = ap.parse_args(argv)
    import torch
    from learn_region_grow_amd import stage, workloads
    if not torch.cuda.is_available():
        raise SystemExit('stage_bench.py needs a GPU: a timing taken without one says nothing')
    rooms = workloads.area5_rooms(args.rooms, cache_dir=args.cache_dir)
    n_points = [len(r['points']) for r in rooms]

    # ---- host path ----
    host_s, host_tuples = [], 0
    for _ in range(args.host_repeats):
        t0 = time.perf_counter()
        rs = np.random.RandomState(args.seed)
        st = stage.center_tuples(stage.merge([stage.stage_room(r['points'], r['obj_id'], rs) for r in rooms]))
        host_s.append(time.perf_counter() - t0)
        host_tuples = len(st['points'])

    # ---- device path ----
    info = {}
    stage.stage_rooms_gpu(rooms, seed=args.seed, info=info)                    # warm-up: code object, allocator
    gpu_s, teacher_ms, tuples_ms = [], [], []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = stage.stage_rooms_gpu(rooms, seed=args.seed, info=info)
        gpu_s.append(time.perf_counter() - t0)
        teacher_ms.append(info['teacher_ms'])
        tuples_ms.append(info['tuples_ms'])
    gpu_tuples = len(st['points'])
    rows = int(sum(len(p) for p in st['points']) + sum(len(p) for p in st['neighbor_points']))
    res = dict(
        workload='%d Area-5-shaped rooms (learn_region_grow_amd.workloads.area5_rooms), %d..%d points, %d in all' % (
            len(rooms), min(n_points), max(n_points), sum(n_points)),
        device=torch.cuda.get_device_name(0), max_points=1024,
        host=dict(path='stage.stage_room, legacy draws, + center_tuples', wall_s=spread(host_s), tuples=host_tuples,
                  tuples_per_s=host_tuples / float(np.median(host_s))),
        gpu=dict(path='stage.stage_rooms_gpu, counter draws, end to end (upload, voxelise, teacher, tuples, download)', wall_s=spread(gpu_s),
                 teacher_kernel_ms=spread(teacher_ms), tuples_kernel_ms=spread(tuples_ms), tuples=gpu_tuples, rows=rows,
                 tuples_per_s=gpu_tuples / float(np.median(gpu_s)), bytes_downloaded=int(info['bytes_downloaded']),
                 teacher_launches=int(info['launches']), rooms_overflowed=len(info['overflowed'])),
        host_over_gpu_wall=float(np.median(host_s) / np.median(gpu_s)),
        note='different random streams: the two paths stage different tuples of the same distribution; times per room set')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
