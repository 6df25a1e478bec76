#!/usr/bin/env python
"""SemanticKITTI sequences -> a room file of fused scenes -- the reference's ``stage_semantic_kitti.py`` with its command line.

    python stage_semantic_kitti.py -d /data/semantic_kitti -o data/kitti_val.h5 -s 08
    python stage_semantic_kitti.py -d /data/semantic_kitti -o data/kitti_train_00.h5 -s 00

Every `interval` consecutive scans are put into the world frame, coloured from the camera images, downsampled and labelled (instance ids
of the dataset, connected components for the rest), on the GPU (learn_region_grow_amd.kitti).  The flags and their short
forms are the reference's; --distance-span is accepted and unused, as there; unknown arguments are tolerated.  The two printed lines are
the reference's.  semantic-kitti.yaml is not needed (the reference reads it and uses nothing from it).  The output is written by
io.saveToH5, so io.loadFromH5, region_grow.py --area kitti_val and stage_data.py --area kitti_train read it.
"""
import argparse
import os
import sys


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--dataset', '-d', type=str, required=True, help='the directory that holds sequences/')
    ap.add_argument('--output', '-o', type=str, required=True, help='room file to write')
    ap.add_argument('--sequences', '-s', type=str, default='00,01,02,03,04,05,06,07,08,09,10')
    ap.add_argument('--interval', '-i', type=int, default=20, help='scans per sample')
    ap.add_argument('--min-cluster', '-m', type=int, default=50, help='a component gets an id when it has more nodes than this')
    ap.add_argument('--voxel-resolution', '-v', type=float, default=0.3)
    ap.add_argument('--downsample-resolution', '-r', type=float, default=0.1)
    ap.add_argument('--distance-span', '-p', type=float, default=50.0, help='unused')
    ap.add_argument('--skip', '-k', type=int, default=10, help='stacks left out between two samples')
    ap.add_argument('--device', default='cuda:0')
    args, _ = ap.parse_known_args(argv)
    return args


def main(argv=None):
    args = parse(argv)
    from learn_region_grow_amd import io as lio
    from learn_region_grow_amd import kitti

    def log(line):
        print(line)
        sys.stdout.flush()
    rooms = kitti.stage_sequences(args.dataset, args.sequences.split(','), interval=args.interval, skip=args.skip, min_cluster=args.min_cluster,
                                  voxel_resolution=args.voxel_resolution, downsample_resolution=args.downsample_resolution, device=args.device,
                                  log=log)
    if os.path.dirname(args.output):
        os.makedirs(os.path.dirname(args.output), exist_ok=True)
    lio.saveToH5(args.output, rooms)


if __name__ == '__main__':
    main()
