#!/usr/bin/env python3
"""Command-line driver with the job of the reference's ``benchmarks.py`` for its classical region-growing baselines:
modes ``normal``, ``curvature``, ``color``, ``feature``, ``smoothness`` and ``fpfh`` on the GPU, the reference's per-room timing and
metric lines and its aggregate line, optional PLY export.

    python baselines.py --area 5 --mode smoothness          # data/s3dis_area5.h5 (benchmarks.py:187-190)
    python baselines.py --h5 rooms.h5 --mode normal --threshold 0.995 --save out/

The rooms of a file go to the GPU in batches (--batch-rooms per lrg_baseline_segment call); features are computed per room
(device equalisation and covariances, host numpy.linalg.svd: learn_region_grow_amd.baselines.room_features).  The timing line
of a room is its feature time plus its share, by equalised points, of its batch's segmentation time.  --features verified solves
the 3x3 decompositions on the GPU too and sends only the points whose labels or rank could depend on the solver through LAPACK: the
same lines, several times faster in the modes that read normals.  Mode pointnet2 of
benchmarks.py is pointnet2.py and mode pointnet is pointnet.py (§3.12).  Mode fpfh computes its descriptor on the GPU
with the arithmetic of PCL's FPFHEstimation, not with PCL's command-line tools (§3.15); its time goes into the batch's segmentation
time.  Mode edge is not ported.
"""
import argparse
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def parse(argv=None):
    from learn_region_grow_amd.baselines import ALL_MODES
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--mode', default='normal', choices=ALL_MODES)
    ap.add_argument('--area', default='1,2,3,4,5,6,scannet', help="comma list of areas: 'scannet', 's3dis', 'kitti_train', ... or an S3DIS area number")
    ap.add_argument('--h5', default=None, help='room file (overrides --area for the data; the area still names the lines)')
    ap.add_argument('--data-dir', default='data')
    ap.add_argument('--threshold', type=float, default=None, help="overrides the mode's first threshold (benchmarks.py:119)")
    ap.add_argument('--resolution', type=float, default=0.1)
    ap.add_argument('--save', nargs='?', const='', default=None, help='write <dir>/<n>.ply per room (default dir: data/results/<mode>)')
    ap.add_argument('--room-names', default=None, help='one room name per line, in file order (data/<area>_room_name.txt)')
    ap.add_argument('--max-rooms', type=int, default=0)
    ap.add_argument('--batch-rooms', type=int, default=68, help='rooms per segmentation call')
    ap.add_argument('--device', default=None, help='default: cuda:0')
    ap.add_argument('--features', default='lapack', choices=('lapack', 'verified'),
                    help="3x3 decompositions: 'lapack' = numpy.linalg.svd for every point on the host; 'verified' = on the GPU, LAPACK only "
                         'for the points the certificate names (same labels)')
    ap.add_argument('--metrics', default='host', choices=('host', 'device'),
                    help="the per-room evaluation: 'host' = metrics.room_metrics room by room; 'device' = all rooms of a segmentation call in one "
                         'pass on the GPU (metrics_gpu.room_metrics_batch)')
    ap.add_argument('--ply-encoder', default='host', choices=('host', 'device'),
                    help="--save: 'host' = io.savePLY, one vertex line per Python iteration; 'device' = the lines encoded on the GPU "
                         '(io.savePLY_device: the same files and printed lines)')
    return ap.parse_args(argv)


def area_file(args, area):
    if args.h5:
        return args.h5
    if area in ('scannet', 's3dis', 'kitti_train', 'kitti_val', 'kitti_small'):
        return os.path.join(args.data_dir, '%s.h5' % area)
    return os.path.join(args.data_dir, 's3dis_area%s.h5' % area)


def room_names(args, area):
    """The room names of an area (benchmarks.py:186-190), or None."""
    name_file = args.room_names or os.path.join(args.data_dir, '%s_room_name.txt' % area)
    if os.path.exists(name_file):
        return open(name_file).read().split('\n')
    return None


def report_room(args, mode, area, r, names, raw_points, seconds, m, unequalized_idx, save_id):
    """The lines benchmarks.py prints for a room of any mode (its timing line, then the metric line) and, with --save, the room's
    PLY coloured by cluster (default dir: data/results/<mode>).  Returns the next save id.  Shared with pointnet2.py."""
    from learn_region_grow_amd import io, metrics
    print('%s %d points: %.2fs' % (names[r] if names is not None and r < len(names) else '', len(raw_points), seconds))
    print(metrics.room_line(area, r, m))
    if args.save is None:
        return save_id
    out_dir = args.save or os.path.join(args.data_dir, 'results', mode)
    os.makedirs(out_dir, exist_ok=True)
    pts = np.array(raw_points[:, :6], dtype=np.float64)
    colors = io.label_colors(int(m['cluster_label2'].max()) + 1)
    pts[:, 3:6] = colors[m['cluster_label2'], :][unequalized_idx]
    save = io.savePLY_device if getattr(args, 'ply_encoder', 'host') == 'device' else io.savePLY
    save(os.path.join(out_dir, ('scannet%d.ply' if area == 'scannet' else '%d.ply') % save_id), pts)
    return save_id + 1


def main(argv=None):
    args = parse(argv)
    from learn_region_grow_amd import baselines, io, metrics
    if args.mode == 'fpfh' and args.features == 'verified':
        sys.exit("--mode fpfh needs --features lapack: no certificate covers the descriptor (DESIGN.md §3.15)")
    areas = args.area.split(',')
    t = list(baselines.default_thresholds(args.mode, areas[0]))
    if args.threshold is not None:
        t[0] = args.threshold
    print('Using threshold', t[0], 'resolution', args.resolution)
    need_normals = args.mode != 'color'
    ms = []
    save_id = 0
    for area in areas:
        rooms, obj_ids, _ = io.loadFromH5(area_file(args, area))
        if args.max_rooms:
            rooms = rooms[:args.max_rooms]
        names = room_names(args, area)
        for b0 in range(0, len(rooms), max(1, args.batch_rooms)):
            batch = range(b0, min(len(rooms), b0 + max(1, args.batch_rooms)))
            feats, ftime = [], []
            for r in batch:
                t0 = time.time()
                feats.append(baselines.room_features(rooms[r], resolution=args.resolution, need_normals=need_normals, device=args.device,
                                                     eig=args.features))
                ftime.append(time.time() - t0)
            t0 = time.time()
            labels = baselines.segment(feats, args.mode, resolution=args.resolution, device=args.device, thresholds=t)
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
                save_id = report_room(args, args.mode, area, r, names, rooms[r], ftime[j] + seg * len(f['points']) / total, m,
                                      f['unequalized_idx'], save_id)
    if ms:
        print(metrics.aggregate_line(ms))
    return 0


if __name__ == '__main__':
    sys.exit(main())
