#!/usr/bin/env python3
"""Command-line driver with the job of the reference's ``test_mcpnet.py``: MCPNet embeddings on the GPU, clustering of the
26-neighbour voxel graph where neighbouring embeddings agree, and the reference's per-room and aggregate lines.

    python mcpnet.py --area 5 --ckpt path/to/mcpnet_model5.ckpt         # data/s3dis_area5.h5 (test_mcpnet.py:56-59)
    python mcpnet.py --h5 rooms.h5 --area 5 --ckpt m.ckpt --rng counter --save out/

The checkpoint is read from where the user names it (default models/mcpnet_model<AREA>.ckpt, mcpnet_model5 for scannet, as at
:50-53); no weights ship with the package.  Rooms go to the GPU in batches of --batch-rooms for the candidate lists, the network
and the clustering.  --rng legacy (the default) draws the neighbour rows on the host from one numpy RandomState(0) running through
every room of every area, as the reference's global stream does; --rng counter draws them on the device.
--save writes <dir>/embedding/<n>.ply and <dir>/results/<n>.ply (default dir: data) as :184-193 does.
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--area', default='1,2,3,4,5,6,scannet', help="comma list of areas: S3DIS area numbers or 'scannet'")
    ap.add_argument('--h5', default=None, help='room file (overrides --area for the data; the area still names the lines and the model)')
    ap.add_argument('--data-dir', default='data')
    ap.add_argument('--ckpt', default=None, help='checkpoint prefix (default models/mcpnet_model<AREA>.ckpt; mcpnet_model5 for scannet)')
    ap.add_argument('--save', nargs='?', const='', default=None, help='write <dir>/embedding/<n>.ply and <dir>/results/<n>.ply (default dir: --data-dir)')
    ap.add_argument('--rng', default='legacy', choices=('legacy', 'counter'))
    ap.add_argument('--seed', type=int, default=0, help='seed of the neighbour draws (legacy: numpy.random.seed, :15)')
    ap.add_argument('--batch-rooms', type=int, default=68, help='rooms per GPU call')
    ap.add_argument('--device', default=None, help='default: cuda:0')
    ap.add_argument('--metrics', default='host', choices=('host', 'device'),
                    help="the per-room evaluation (:146-170): 'host' = metrics.room_metrics_set_order room by room; 'device' = all rooms of a "
                         "batch in one pass on the GPU (metrics_gpu.room_metrics_batch, order='set')")
    return ap.parse_args(argv)


def model_path(args, area):
    if args.ckpt:
        return args.ckpt
    return 'models/mcpnet_model5.ckpt' if area == 'scannet' else 'models/mcpnet_model%s.ckpt' % area


def area_file(args, area):
    if args.h5:
        return args.h5
    return os.path.join(args.data_dir, 'scannet.h5' if area == 'scannet' else 's3dis_area%s.h5' % area)


def main(argv=None):
    args = parse(argv)
    from learn_region_grow_amd import checkpoint, io, mcpnet, metrics
    state = np.random.RandomState(args.seed)                 # :15, one stream through every room of every area
    ms = []
    save_id = 0
    for area in args.area.split(','):
        path = model_path(args, area)
        net = mcpnet.MCPNetHIP(checkpoint.load_mcpnet_weights(path), device=args.device)
        print('Restored from %s' % path)
        raw_rooms, obj_ids, _ = io.loadFromH5(area_file(args, area))
        step = max(1, args.batch_rooms)
        for b0 in range(0, len(raw_rooms), step):
            batch = list(range(b0, min(len(raw_rooms), b0 + step)))
            rooms = [mcpnet.prepare_room(raw_rooms[r], room_id=r, device=args.device) for r in batch]
            nbrs = mcpnet.neighbors(rooms, rng=args.rng, seed=args.seed, state=state, device=args.device)
            embs = net.embed([r['points'] for r in rooms], nbrs)
            labels = mcpnet.segment(rooms, embs, device=args.device)
            room_ms = None
            if args.metrics == 'device':
                from learn_region_grow_amd import metrics_gpu
                room_ms = metrics_gpu.room_metrics_batch([obj_ids[r][rooms[j]['equalized_idx']] for j, r in enumerate(batch)],
                                                         [lab.astype(np.int64) for lab in labels], order='set', device=args.device)
            for j, r in enumerate(batch):
                lab = labels[j].astype(np.int64)
                m = room_ms[j] if room_ms is not None else metrics.room_metrics_set_order(obj_ids[r][rooms[j]['equalized_idx']], lab)
                ms.append(m)
                print(metrics.room_line(area, r, m))
                if args.save is not None:
                    out_dir = args.save or args.data_dir
                    os.makedirs(os.path.join(out_dir, 'embedding'), exist_ok=True)
                    os.makedirs(os.path.join(out_dir, 'results'), exist_ok=True)
                    pts = np.array(rooms[j]['centred'], dtype=np.float32)
                    uq = rooms[j]['unequalized_idx']
                    pts[:, 3:6] = mcpnet.embedding_colors(embs[j])[uq]
                    io.savePLY(os.path.join(out_dir, 'embedding', '%d.ply' % save_id), pts)
                    pts[:, 3:6] = mcpnet.result_colors(m['cluster_label2'])[uq]
                    io.savePLY(os.path.join(out_dir, 'results', '%d.ply' % save_id), pts)
                    save_id += 1
    if ms:
        print(metrics.aggregate_line(ms))
    return 0


if __name__ == '__main__':
    sys.exit(main())
