#!/usr/bin/env python3
"""Command-line driver with the job of the reference's ``benchmarks.py --mode pointnet2``: PointNet2 classes of every equalised
point on the GPU (cells of 1024 rows, benchmarks.py:281-298), clustering of the 26-neighbour voxel graph where neighbouring classes
are equal, and the reference's per-room timing and metric lines and its aggregate line, optional PLY export.

    python pointnet2.py --area 5 --ckpt path/to/pointnet2_model5.ckpt         # data/s3dis_area5.h5 (benchmarks.py:182-185)
    python pointnet2.py --h5 scenes.h5 --area kitti_val --ckpt m.ckpt --save out/

The checkpoint is read from where the user names it (default models/pointnet2_model<AREA>.ckpt, pointnet2_model5 for scannet, as
at :156-161); no weights ship with the package.  Its shapes say whether the network reads colour features and how many classes
it has.  The rooms of a file go to the GPU in batches of --batch-rooms: all their cells pass through the network together, and one
segmentation call labels them.  An area whose name contains 'kitti' is cut into 3 m cells, any other into 1 m
cells (:283).  The timing line of a room is its equalisation time plus its share, by equalised points, of its batch's network
and segmentation time.
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

MODE = 'pointnet2'


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--area', default='1,2,3,4,5,6,scannet', help="comma list of areas: 'scannet', 's3dis', 'kitti_train', ... or an S3DIS area number")
    ap.add_argument('--h5', default=None, help='room file (overrides --area for the data; the area still names the lines, the model and the cell size)')
    ap.add_argument('--data-dir', default='data')
    ap.add_argument('--ckpt', default=None, help='checkpoint prefix (default models/pointnet2_model<AREA>.ckpt; pointnet2_model5 for scannet)')
    ap.add_argument('--save', nargs='?', const='', default=None, help='write <dir>/<n>.ply per room (default dir: data/results/pointnet2)')
    ap.add_argument('--room-names', default=None, help='one room name per line, in file order (data/<area>_room_name.txt)')
    ap.add_argument('--max-rooms', type=int, default=0)
    ap.add_argument('--batch-rooms', type=int, default=68, help='rooms per network and segmentation call')
    ap.add_argument('--device', default=None, help='default: cuda:0')
    ap.add_argument('--metrics', default='host', choices=('host', 'device'),
                    help="the per-room evaluation: 'host' = metrics.room_metrics room by room; 'device' = all rooms of a batch in one "
                         'pass on the GPU (metrics_gpu.room_metrics_batch)')
    return ap.parse_args(argv)


def model_path(args, area):
    if args.ckpt:
        return args.ckpt
    return 'models/pointnet2_model5.ckpt' if area == 'scannet' else 'models/pointnet2_model%s.ckpt' % area


def main(argv=None):
    args = parse(argv)
    import baselines as cli                                   # the room files, room names and per-room report of baselines.py
    from learn_region_grow_amd import checkpoint, io, metrics, pointnet2
    ms = []
    save_id = 0
    for area in args.area.split(','):
        path = model_path(args, area)
        net = pointnet2.PointNet2HIP(checkpoint.load_pointnet2_weights(path), device=args.device)
        print('Restored from %s' % path)
        rooms, obj_ids, _ = io.loadFromH5(cli.area_file(args, area))
        if args.max_rooms:
            rooms = rooms[:args.max_rooms]
        names = cli.room_names(args, area)
        step = max(1, args.batch_rooms)
        for b0 in range(0, len(rooms), step):
            batch = range(b0, min(len(rooms), b0 + step))
            feats, ftime = [], []
            for r in batch:
                t0 = time.time()
                feats.append(dict(pointnet2.prepare_room(rooms[r], device=args.device), room_id=r))
                ftime.append(time.time() - t0)
            t0 = time.time()
            classes = net.classify(feats, area=area)
            labels = pointnet2.segment(feats, classes, device=args.device)
            seg = time.time() - t0
            total = max(1, sum(len(f['points']) for f in feats))
            room_ms = None
            if args.metrics == 'device':
                from learn_region_grow_amd import metrics_gpu
                room_ms = metrics_gpu.room_metrics_batch([obj_ids[r][feats[j]['equalized_idx']] for j, r in enumerate(batch)],
                                                         [lab.astype(np.int64) for lab in labels], device=args.device)
            for j, r in enumerate(batch):
                f, lab = feats[j], labels[j].astype(np.int64)
                m = room_ms[j] if room_ms is not None else metrics.room_metrics(obj_ids[r][f['equalized_idx']], lab)
                ms.append(m)
                save_id = cli.report_room(args, MODE, area, r, names, rooms[r], ftime[j] + seg * len(f['points']) / total, m,
                                          f['unequalized_idx'], save_id)
    if ms:
        print(metrics.aggregate_line(ms))
    return 0


if __name__ == '__main__':
    sys.exit(main())
