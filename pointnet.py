#!/usr/bin/env python3
"""Command-line driver with the job of the reference's ``benchmarks.py --mode pointnet``: plain PointNet classes of every equalised
point on the GPU (cells of 1024 rows, benchmarks.py:281-298), clustering of the 26-neighbour voxel graph where neighbouring classes
are equal, and the reference's per-room timing and metric lines and its aggregate line, optional PLY export.

    python pointnet.py --area 5 --ckpt path/to/pointnet_model5.ckpt           # data/s3dis_area5.h5 (benchmarks.py:182-185)
    python pointnet.py --h5 scenes.h5 --area kitti_val --ckpt m.ckpt --save out/

The checkpoint is read from where the user names it (default models/pointnet_model<AREA>.ckpt, pointnet_model5 for scannet, as at
:156-161); no weights ship with the package.  Its shapes say which network it holds: the convolutions' and fc layers' widths and
the class count (the shipped pointnet_model5 is not the network train_pointnet.py builds today; both run).  Everything but the
network is pointnet2.py's: the rooms of a file go to the GPU in batches of --batch-rooms, all their cells pass through the network
together, and one segmentation call labels them.
"""
import os
import sys

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

MODE = 'pointnet'


def parse(argv=None):
    from learn_region_grow_amd import classifier_cli
    return classifier_cli.parse(argv, MODE, __doc__)


def model_path(args, area):
    from learn_region_grow_amd import classifier_cli
    return classifier_cli.model_path(args, area, MODE)


def main(argv=None):
    args = parse(argv)
    import baselines as cli                                   # the room files, room names and per-room report of baselines.py
    from learn_region_grow_amd import checkpoint, classifier_cli, pointnet
    return classifier_cli.run(args, MODE, lambda path: pointnet.PointNetHIP(checkpoint.load_pointnet_weights(path), device=args.device), cli)


if __name__ == '__main__':
    sys.exit(main())
