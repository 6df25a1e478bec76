#!/usr/bin/env python
"""Training tuples for LrgNet from labelled rooms -- the reference's ``stage_data.py`` with its command line and file names.

    python stage_data.py --area 1,2,3,4,5,6 --seed 3        # = stage_data.py --seed 3 --area 1,2,3,4,5,6
    python stage_data.py --area synthetic_train             # data/synthetic_train.h5 -> data/staged_synthetic_train.h5

Kept from the reference: --seed, --area (comma list), --resolution; the inputs of stage_data.py:27-34 and the outputs of :242-248
(data/staged_<synthetic*>.h5, data/staged_area<a>.h5 without --seed, data/multiseed/seed<k>_area<a>.h5 with it), read by
train_region_grow.py.  --seed also selects the augmentation of :50-56 (learn_region_grow_amd.stage.seed_transform).

--rng counter (default): the device teacher (lrg_stage_teacher / lrg_stage_tuples), all rooms of a file in one launch, draws keyed by
(seed, room).  --rng legacy: the reference's stream -- ONE RandomState(seed or 0) for all rooms of all areas of the call, in file order
(the reference seeds once, :13/:18, and never reseeds) -- on the host; with --preprocess host this path needs no GPU.
"""
import argparse
import os
import sys

import numpy as np

NAMED_AREAS = ('s3dis', 'scannet', 'kitti_val', 'kitti_train')


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--seed', type=int, default=None, help='0..7: the augmentation of stage_data.py:50-56 and the generator seed; output under data/multiseed/')
    ap.add_argument('--area', default='1,2,3,4,5,6', help="comma list of 1..6, s3dis, scannet, kitti_val, kitti_train, synthetic*")
    ap.add_argument('--resolution', type=float, default=0.1)
    ap.add_argument('--h5', default=None, help='room file (overrides the input name of --area; one area only)')
    ap.add_argument('--out', default=None, help='staged file (overrides the output name; one area only)')
    ap.add_argument('--data-dir', default='data')
    ap.add_argument('--max-rooms', type=int, default=0)
    ap.add_argument('--rng', default='counter', choices=['legacy', 'counter'])
    ap.add_argument('--preprocess', default='gpu-exact', choices=['gpu-exact', 'host'],
                    help="equalisation / normals / curvature (stage_data.py:58-102): 'gpu-exact' = preprocess_gpu.preprocess_rooms, one batched pass")
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--max-points', type=int, default=1024, help='points per side of a tuple (stage_data.py:11)')
    ap.add_argument('--quiet', action='store_true', help='do not print the per-object lines (stage_data.py:206)')
    args = ap.parse_args(argv)
    args.areas = args.area.split(',')
    for a in args.areas:
        if not (a in ('1', '2', '3', '4', '5', '6') or a in NAMED_AREAS or a.startswith('synthetic')):
            ap.error('unknown area %r' % a)
        if a == 'kitti_train' and args.seed is None:
            ap.error('kitti_train reads data/kitti_train_<seed>.h5: give --seed')
    if (args.h5 or args.out) and len(args.areas) != 1:
        ap.error('--h5 / --out name one file: give one area')
    if args.seed is not None and args.seed < 0:
        ap.error('--seed must not be negative')
    return args


def input_path(args, area):
    """stage_data.py:27-34."""
    if args.h5:
        return args.h5
    if area.startswith('synthetic') or area in ('s3dis', 'scannet', 'kitti_val'):
        return os.path.join(args.data_dir, '%s.h5' % area)
    if area == 'kitti_train':
        return os.path.join(args.data_dir, '%s_%02d.h5' % (area, args.seed))
    return os.path.join(args.data_dir, 's3dis_area%s.h5' % area)


def output_path(args, area):
    """stage_data.py:242-248."""
    if args.out:
        return args.out
    if area.startswith('synthetic'):
        return os.path.join(args.data_dir, 'staged_%s.h5' % area)
    if args.seed is None:
        return os.path.join(args.data_dir, 'staged_area%s.h5' % area)
    return os.path.join(args.data_dir, 'multiseed', 'seed%d_area%s.h5' % (args.seed, area))


def object_lines(area, room_id, room, objects, resolution):
    """The lines of stage_data.py:206 for the stored objects of one room of the device teacher."""
    obj_id = np.asarray(room['obj_id'])
    vox = np.round(np.asarray(room['points'])[:, :3] / resolution).astype(int)
    out = []
    for steps, seed, count, iou_bits in objects:
        gt = obj_id == obj_id[seed]
        lo, hi = vox[gt].min(axis=0), vox[gt].max(axis=0)                                          # :112-118
        box = np.logical_and(np.all(vox >= lo, axis=1), np.all(vox <= hi, axis=1))
        original = 1.0 * np.sum(np.logical_and(gt, box)) / np.sum(np.logical_or(gt, box))
        iou = float(np.array([iou_bits], dtype=np.int32).view(np.float32)[0])
        out.append('AREA %s room %d target %d: %d steps %d/%d (%.2f/%.2f IOU)' % (area, room_id, obj_id[seed], steps, count, int(gt.sum()), iou, original))
    return out


def main(argv=None):
    args = parse(argv)
    from learn_region_grow_amd import io as lio
    from learn_region_grow_amd import preprocess, stage
    rs = np.random.RandomState(args.seed or 0) if args.rng == 'legacy' else None               # :13, :18: seeded once for the whole call
    for area in args.areas:
        all_points, all_obj_id, all_cls_id = lio.loadFromH5(input_path(args, area))
        n_rooms = min(len(all_points), args.max_rooms) if args.max_rooms else len(all_points)
        raw = [(stage.seed_transform(all_points[r], args.seed), all_obj_id[r], all_cls_id[r]) for r in range(n_rooms)]    # :50-56
        if args.preprocess == 'host':
            pre = [preprocess.preprocess_room(p, o, c, resolution=args.resolution) for p, o, c in raw]
        else:
            from learn_region_grow_amd import preprocess_gpu
            pre = preprocess_gpu.preprocess_rooms(raw, resolution=args.resolution, eig='exact', device=args.device) if raw else []
        rooms = [dict(points=p['points'], obj_id=p['obj_id'], room_id=r) for r, p in enumerate(pre)]
        if args.rng == 'legacy':
            parts = []
            for r, room in enumerate(rooms):
                log = None if args.quiet else (lambda s, r=r: print('AREA %s room %d %s' % (area, r, s)))
                parts.append(stage.stage_room(room['points'], room['obj_id'], rs, resolution=args.resolution, max_points=args.max_points, log=log))
            staged = stage.center_tuples(stage.merge(parts))
        else:
            info = {}
            staged = stage.stage_rooms_gpu(rooms, seed=args.seed or 0, resolution=args.resolution, max_points=args.max_points, device=args.device,
                                           info=info)
            if not args.quiet:
                for r, room in enumerate(rooms):
                    for line in object_lines(area, r, room, info['objects'][r], args.resolution):
                        print(line)
        path = output_path(args, area)
        if os.path.dirname(path):
            os.makedirs(os.path.dirname(path), exist_ok=True)
        stage.save_staged(path, staged)
        print('AREA %s: %d rooms, %d tuples, %d objects -> %s' % (area, len(rooms), len(staged['points']), len(staged['steps']), path))
        sys.stdout.flush()


if __name__ == '__main__':
    main()
