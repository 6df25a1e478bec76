#!/usr/bin/env python3
"""Command-line driver with the job of the reference's ``benchmarks.py --mode edge``: the pickled edge classifier on every edge of
the 26-neighbour voxel graph, clusters of the edges it keeps, the fallback search for the points left over, and the reference's
per-room timing and metric lines and its aggregate line.

    python edge.py --area 5 --ckpt path/to/models/edge5.pkl               # data/s3dis_area5.h5
    python edge.py --h5 rooms.h5 --area 5 --ckpt models/edge5.pkl --save out/

The model is read from where the user names it (default models/edge<AREA>.pkl, edge5 for scannet, as benchmarks.py:174-178); an
.npz of its eight arrays is accepted too; no weights ship with the package.  --sigmoid host (the default) sends the logits through
scipy.special.expit on the host, the function the reference's sklearn calls; --sigmoid device keeps them on the GPU (DESIGN.md
§3.16 says what that can change).  --save writes <dir>/<n>.ply per room (default dir: data/results/edge).
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
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--area', default='1,2,3,4,5,6,scannet', help="comma list of areas: 'scannet', 's3dis', 'kitti_train', ... or an S3DIS area number")
    ap.add_argument('--h5', default=None, help='room file (overrides --area for the data; the area still names the lines and the model)')
    ap.add_argument('--data-dir', default='data')
    ap.add_argument('--ckpt', default=None, help='the classifier: a joblib pickle or an .npz (default models/edge<AREA>.pkl; edge5 for scannet)')
    ap.add_argument('--resolution', type=float, default=0.1)
    ap.add_argument('--sigmoid', default='host', choices=('host', 'device'))
    ap.add_argument('--save', nargs='?', const='', default=None, help='write <dir>/<n>.ply per room (default dir: data/results/edge)')
    ap.add_argument('--room-names', default=None, help='one room name per line, in file order (data/<area>_room_name.txt)')
    ap.add_argument('--max-rooms', type=int, default=0)
    ap.add_argument('--batch-rooms', type=int, default=68, help='rooms per GPU call')
    ap.add_argument('--device', default=None, help='default: cuda:0')
    ap.add_argument('--metrics', default='host', choices=('host', 'device'),
                    help="the per-room evaluation: 'host' = metrics.room_metrics room by room; 'device' = all rooms of a batch in one pass on "
                         'the GPU (metrics_gpu.room_metrics_batch)')
    ap.add_argument('--ply-encoder', default='host', choices=('host', 'device'),
                    help="--save: 'host' = io.savePLY, one vertex line per Python iteration; 'device' = the lines encoded on the GPU "
                         '(io.savePLY_device: the same files and printed lines)')
    return ap.parse_args(argv)


def model_path(args, area):
    if args.ckpt:
        return args.ckpt
    return 'models/edge5.pkl' if area == 'scannet' else 'models/edge%s.pkl' % area


def main(argv=None):
    args = parse(argv)
    import baselines as driver                                     # area_file, room_names, report_room: the lines of every benchmarks.py mode
    from learn_region_grow_amd import baselines, edge, io, metrics
    ms = []
    save_id = 0
    for area in args.area.split(','):
        path = model_path(args, area)
        model = edge.EdgeModelHIP(edge.load_edge_model(path), device=args.device)
        print('Restored from %s' % path)
        rooms, obj_ids, _ = io.loadFromH5(driver.area_file(args, area))
        if args.max_rooms:
            rooms = rooms[:args.max_rooms]
        names = driver.room_names(args, area)
        step = max(1, args.batch_rooms)
        for b0 in range(0, len(rooms), step):
            batch = range(b0, min(len(rooms), b0 + step))
            feats, ftime = [], []
            for r in batch:
                t0 = time.time()
                feats.append(baselines.room_features(rooms[r], resolution=args.resolution, need_normals=False, device=args.device))
                ftime.append(time.time() - t0)
            t0 = time.time()
            labels = edge.segment(feats, model, resolution=args.resolution, sigmoid=args.sigmoid)
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
                save_id = driver.report_room(args, 'edge', area, r, names, rooms[r], ftime[j] + seg * len(f['points']) / total, m,
                                             f['unequalized_idx'], save_id)
    if ms:
        print(metrics.aggregate_line(ms))
    return 0


if __name__ == '__main__':
    sys.exit(main())
