"""Room by room against all rooms in one pass: preprocess_gpu.preprocess_room in a loop and preprocess_gpu.preprocess_rooms on the 68
Area-5-shaped rooms of bench.py's p0_rates (synthetic.AREA5_POINTS, seeds 9000 + i), host memory in / host memory out.

Per eig mode: first the two must agree on every room (points, order, obj_id, equalized_idx, unequalized_idx bit for bit); both are warmed;
then the loop and the batch alternate, --repeats samples each, a host clock around work that ends in a device synchronise.  Written
out: rooms/s of both with every sample, and the batch's split (device pass, copies, LAPACK, argsort, the rest) summed over its samples.

    python tools/prep_batch_bench.py --out profiles/prep_batch.json
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/prep_batch_bench.py --modes jacobi --repeats 1 --no-check --out ''
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rooms', type=int, default=68)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--modes', default='jacobi,exact,lapack')
    ap.add_argument('--no-check', action='store_true')
    ap.add_argument('--out', default='profiles/prep_batch.json')
    args = ap.parse_args()
    import torch
    from learn_region_grow_amd import preprocess_gpu, synthetic
    dev = torch.device('cuda:0')
    targets = [synthetic.AREA5_POINTS[(7 * i) % len(synthetic.AREA5_POINTS)] for i in range(args.rooms)]
    raws = []
    for i, t in enumerate(targets):
        r = synthetic.area5_shaped_room(t, 9000 + i).astype(np.float32)
        raws.append((r[:, :6], r[:, 6].astype(int), r[:, 7].astype(int)))
    print('%d rooms, %d raw points' % (len(raws), sum(len(r[0]) for r in raws)), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), rooms=len(raws), raw_points=[len(r[0]) for r in raws], repeats=args.repeats, modes={})

    def loop(eig):
        return [preprocess_gpu.preprocess_room(*raw, eig=eig, device=dev) for raw in raws]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    for eig in args.modes.split(','):
        want, got = loop(eig), preprocess_gpu.preprocess_rooms(raws, eig=eig, device=dev)          # (warms both)
        if not args.no_check:
            for k, (g, w) in enumerate(zip(got, want)):
                for key in ('points', 'order', 'obj_id', 'equalized_idx', 'unequalized_idx'):
                    assert g[key].dtype == w[key].dtype and np.array_equal(g[key], w[key], equal_nan=key == 'points'), (eig, k, key)
        equalized = int(sum(len(g['points']) for g in got))
        lapack_points = int(sum(g['exact_stats']['lapack_points'] for g in got)) if eig == 'exact' else (equalized if eig == 'lapack' else 0)
        del want, got
        t_loop, t_batch, split = [], [], {}
        for _ in range(args.repeats):
            t_loop.append(timed(lambda: loop(eig)))
            t_batch.append(timed(lambda: preprocess_gpu.preprocess_rooms(raws, eig=eig, device=dev, timing=split)))
        n = len(raws)
        total = split.pop('total')
        split['rest'] = total - sum(split.values())
        res = dict(loop_rooms_per_sec=n / float(np.median(t_loop)), batch_rooms_per_sec=n / float(np.median(t_batch)),
                   loop_samples_rooms_per_sec=[n / t for t in t_loop], batch_samples_rooms_per_sec=[n / t for t in t_batch],
                   batch_median_beats_loop_best=bool(np.median(t_batch) < min(t_loop)),
                   batch_split_seconds_per_run={k: v / args.repeats for k, v in sorted(split.items())},
                   batch_seconds_per_run=total / args.repeats, equalized_points=equalized, lapack_points=lapack_points)
        out['modes'][eig] = res
        print(eig, json.dumps(res), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
