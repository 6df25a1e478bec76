"""What the command lines of the two learned per-point classifiers share (``pointnet.py`` and ``pointnet2.py`` in the repository's
root: the reference's ``benchmarks.py --mode pointnet`` / ``--mode pointnet2``).  The modes differ in the network only: the
equalisation, the xy cells of 1024 rows, the class-agreement edges on the 26-neighbour voxel graph, the metric lines and the PLYs
are the same (benchmarks.py:199-215, :281-306, :405-416).

``parse``        the arguments; the mode's name appears in two help strings.
``model_path``   the default checkpoint, models/<mode>_model<AREA>.ckpt (<mode>_model5 for scannet, as at :156-161).
``run``          the loop over areas and room batches, given a function that builds the network from a checkpoint prefix.
"""
import argparse
import time

import numpy as np


def parse(argv, mode, doc):
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--area', default='1,2,3,4,5,6,scannet', help="comma list of areas: 'scannet', 's3dis', 'kitti_train', ... or an S3DIS area number")
    ap.add_argument('--h5', default=None, help='room file (overrides --area for the data; the area still names the lines, the model and the cell size)')
    ap.add_argument('--data-dir', default='data')
    ap.add_argument('--ckpt', default=None, help='checkpoint prefix (default models/%s_model<AREA>.ckpt; %s_model5 for scannet)' % (mode, mode))
    ap.add_argument('--save', nargs='?', const='', default=None, help='write <dir>/<n>.ply per room (default dir: data/results/%s)' % mode)
    ap.add_argument('--room-names', default=None, help='one room name per line, in file order (data/<area>_room_name.txt)')
    ap.add_argument('--max-rooms', type=int, default=0)
    ap.add_argument('--batch-rooms', type=int, default=68, help='rooms per network and segmentation call')
    ap.add_argument('--device', default=None, help='default: cuda:0')
    ap.add_argument('--metrics', default='host', choices=('host', 'device'),
                    help="the per-room evaluation: 'host' = metrics.room_metrics room by room; 'device' = all rooms of a batch in one "
                         'pass on the GPU (metrics_gpu.room_metrics_batch)')
    ap.add_argument('--ply-encoder', default='host', choices=('host', 'device'),
                    help="--save: 'host' = io.savePLY, one vertex line per Python iteration; 'device' = the lines encoded on the GPU "
                         '(io.savePLY_device: the same files and printed lines)')
    return ap.parse_args(argv)


def model_path(args, area, mode):
    if args.ckpt:
        return args.ckpt
    return 'models/%s_model5.ckpt' % mode if area == 'scannet' else 'models/%s_model%s.ckpt' % (mode, area)


def run(args, mode, build_net, cli):
    """build_net(checkpoint prefix) -> an object with classify(rooms, area=...) (PointNetHIP, PointNet2HIP); cli: the root
    ``baselines`` module (the room files, room names and per-room report of baselines.py)."""
    from . import io, metrics, pointnet2
    ms = []
    save_id = 0
    for area in args.area.split(','):
        path = model_path(args, area, mode)
        net = build_net(path)
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
                from . import metrics_gpu
                room_ms = metrics_gpu.room_metrics_batch([obj_ids[r][feats[j]['equalized_idx']] for j, r in enumerate(batch)],
                                                         [lab.astype(np.int64) for lab in labels], device=args.device)
            for j, r in enumerate(batch):
                f, lab = feats[j], labels[j].astype(np.int64)
                m = room_ms[j] if room_ms is not None else metrics.room_metrics(obj_ids[r][f['equalized_idx']], lab)
                ms.append(m)
                save_id = cli.report_room(args, mode, area, r, names, rooms[r], ftime[j] + seg * len(f['points']) / total, m,
                                          f['unequalized_idx'], save_id)
    if ms:
        print(metrics.aggregate_line(ms))
    return 0
