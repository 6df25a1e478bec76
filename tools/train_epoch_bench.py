#!/usr/bin/env python
"""Time per LrgNet training step with the batch put together on the host (train_region_grow.run_epoch: stage.assemble_batch, upload,
train_step, two synchronisations a step) against --assemble device (run_epoch_device: TupleStore.assemble + train_step_device, one
synchronisation per window), on the same tuples, the same commit and machine.  Writes profiles/train_epoch_bench.json.

The tuples are those of Area-5-shaped rooms (learn_region_grow_amd.workloads.area5_rooms, as tools/stage_bench.py makes them) staged by the
device teacher; B = 100, 512 + 512 points.  The two paths alternate in one process, window after window of `--window` steps over the same
tuples; each is warmed up by one window first; a window's time is a host clock around work that ends synchronised (the host path
synchronises every step, the device path when it reads its statistics).  Also reported: the two assembly kernels' time by device events,
and what staging the rooms online costs per epoch (stage_rooms_gpu(download=False) + TupleStore.from_device, preprocessing not included:
the workload's rooms come preprocessed) beside the staging that downloads.  The two paths draw different subsets (legacy stream against
counter stream), so the comparison is of time, not of bytes.

    python tools/train_epoch_bench.py [--rooms 16] [--window 50] [--windows 4] [--out profiles/train_epoch_bench.json]
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
    ap.add_argument('--rooms', type=int, default=16)
    ap.add_argument('--batch-size', type=int, default=100)
    ap.add_argument('--window', type=int, default=50, help='steps per timed window')
    ap.add_argument('--windows', type=int, default=4, help='timed windows per path (window * windows >= 200 steps)')
    ap.add_argument('--stage-repeats', type=int, default=3)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--cache-dir', default=None)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'train_epoch_bench.json'))
    args = ap.parse_args(argv)
    import torch
    import train_region_grow
    from learn_region_grow_amd import stage, synthetic, workloads
    from learn_region_grow_amd.train import LrgNetTrainer
    from learn_region_grow_amd.train_data import BatchBuffers, TupleStore
    if not torch.cuda.is_available():
        raise SystemExit('train_epoch_bench.py needs a GPU: a timing taken without one says nothing')
    if args.window * args.windows < 200:
        raise SystemExit('at least 200 timed steps per path')
    B, dev = args.batch_size, 'cuda:0'
    rooms = workloads.area5_rooms(args.rooms, cache_dir=args.cache_dir)
    n_points = [len(r['points']) for r in rooms]

    # ---- staging: downloaded (what a staged file holds) and left on the device ----
    info = {}
    stage.stage_rooms_gpu(rooms, seed=args.seed, info=info)                    # warm-up: code object, allocator
    down_s, left_s = [], []
    for _ in range(args.stage_repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        staged = stage.stage_rooms_gpu(rooms, seed=args.seed, info=info)
        down_s.append(time.perf_counter() - t0)
    bytes_down = int(info['bytes_downloaded'])
    for _ in range(args.stage_repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        store = TupleStore.from_device(stage.stage_rooms_gpu(rooms, seed=args.seed, info=info, download=False)['device'], 13, rng_seed=args.seed)
        torch.cuda.synchronize()
        left_s.append(time.perf_counter() - t0)
    bytes_left = int(info['bytes_downloaded'])
    keep = [i for i in range(len(staged['points'])) if len(staged['neighbor_points'][i]) > 0]
    data = {k: [staged[k][i] for i in keep] for k in ('points', 'remove', 'neighbor_points', 'add')}
    T = len(store)
    assert T == len(keep)
    per_window = args.window * B
    if T < per_window:
        raise SystemExit('%d tuples: fewer than one window of %d steps; give more --rooms' % (T, args.window))

    # ---- the two paths, window after window over the same tuples ----
    trainer = LrgNetTrainer(B, 512, 512, 13, 0, device=dev).load_weights(synthetic.make_reference_init_weights(seed=args.seed))
    bufs = BatchBuffers(B, 512, 512, 13, dev)
    rs_pick = np.random.RandomState(args.seed + 1)

    def window_tuples():
        sel = np.sort(rs_pick.choice(T, per_window, replace=False))
        sub = {k: [data[k][i] for i in sel] for k in data}
        sub_store = TupleStore(store.points, store.remove, store.neighbor_points, store.add, store.start_in[sel], store.count_in[sel],
                               store.start_nb[sel], store.count_nb[sel], 13, rng_seed=args.seed)
        return sub, sub_store

    def host_window(sub, rs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        train_region_grow.run_epoch(trainer, sub, rs, B)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def device_window(sub_store, rs, epoch):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        train_region_grow.run_epoch_device(trainer, sub_store, rs, B, epoch, bufs)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    rs_h, rs_d = np.random.RandomState(args.seed), np.random.RandomState(args.seed)
    sub, sub_store = window_tuples()
    host_window(sub, rs_h)                                                     # warm-up of each path
    device_window(sub_store, rs_d, 0)
    host_ms, device_ms = [], []
    for w in range(args.windows):
        sub, sub_store = window_tuples()
        host_ms.append(1e3 * host_window(sub, rs_h) / args.window)
        device_ms.append(1e3 * device_window(sub_store, rs_d, w + 1) / args.window)

    # ---- the host assembly alone (no GPU work in it) and the assembly kernels by events ----
    rs_a = np.random.RandomState(args.seed)
    idx = np.arange(per_window)
    t0 = time.perf_counter()
    for b in range(args.window):
        stage.assemble_batch(sub, idx[b * B:(b + 1) * B], rs_a, B, 512, 512)
    host_assembly_ms = 1e3 * (time.perf_counter() - t0) / args.window
    order = sub_store.upload_order(idx)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    kernel_ms = []
    for rep in range(4):
        ev[0].record()
        for b in range(args.window):
            sub_store.assemble(order[b * B:(b + 1) * B], rep, 0, bufs)
        ev[1].record()
        ev[1].synchronize()
        if rep:                                                                # the first repeat warms up
            kernel_ms.append(ev[0].elapsed_time(ev[1]) / args.window)

    h, d = float(np.median(host_ms)), float(np.median(device_ms))
    res = dict(
        workload='tuples of %d Area-5-shaped rooms (learn_region_grow_amd.workloads.area5_rooms), %d..%d points; %d kept tuples; B = %d, 512 + 512 '
                 'points, feature size 13, lite 0' % (len(rooms), min(n_points), max(n_points), T, B),
        device=torch.cuda.get_device_name(0), steps_per_window=args.window, windows=args.windows,
        host=dict(path='train_region_grow.run_epoch: stage.assemble_batch (legacy draws) + upload + train_step, two synchronisations a step',
                  step_ms=spread(host_ms), assembly_alone_ms=host_assembly_ms),
        device_path=dict(path='train_region_grow.run_epoch_device: TupleStore.assemble (counter draws) + train_step_device, one synchronisation '
                              'per window', step_ms=spread(device_ms),
                         assemble_kernels_ms=spread(kernel_ms), assemble_kernels_note='both sides of one batch (two lrg_train_assemble launches), by '
                         'device events around %d batches back to back' % args.window),
        host_over_device_step=h / d, device_step_is_lower=bool(d < h),
        staging=dict(downloaded=dict(path='stage.stage_rooms_gpu (rows downloaded and split: what stage_data.py writes)', wall_s=spread(down_s),
                                     bytes_downloaded=bytes_down),
                     online=dict(path='stage.stage_rooms_gpu(download=False) + TupleStore.from_device: the per-epoch cost of --stage online for these '
                                      'rooms, preprocessing not included', wall_s=spread(left_s), bytes_downloaded=bytes_left,
                                 store_bytes=int(store.nbytes()))),
        unmeasured='real S3DIS data; device memory and times at the scale of whole areas; preprocess_rooms in the online epoch',
        note='the two paths draw from different streams: equal distributions, different subsets; times per step, not bytes')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
