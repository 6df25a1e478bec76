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
import os
import sys

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

MODE = 'pointnet2'


def parse(argv=None):
    from learn_region_grow_amd import classifier_cli
    return classifier_cli.parse(argv, MODE, __doc__)


def model_path(args, area):
    from learn_region_grow_amd import classifier_cli
    return classifier_cli.model_path(args, area, MODE)


def main(argv=None):
    args = parse(argv)
    import baselines as cli                                   # the room files, room names and per-room report of baselines.py
    from learn_region_grow_amd import checkpoint, classifier_cli, pointnet2
    return classifier_cli.run(args, MODE, lambda path: pointnet2.PointNet2HIP(checkpoint.load_pointnet2_weights(path), device=args.device), cli)


if __name__ == '__main__':
    sys.exit(main())
