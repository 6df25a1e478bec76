#!/usr/bin/env python3
"""Command-line driver with the job of the reference's ``train_pointnet.py --mode pointnet2``: the twin of ``train_pointnet.py``.
The same rooms cut into the same cells of 2048 rows (:327-350), PointNet++ (:113-211: no batch norm, no dropout, Adam at a constant
0.001) trained on the GPU, the reference's epoch lines, and the weights saved as a TensorFlow checkpoint bundle that
``pointnet2.py --ckpt`` (and the reference's ``Saver.restore``) reads.

    python train_pointnet2.py --train-area 1,2,3,4,6 --val-area 5             # -> models/pointnet2_model5.ckpt
    python train_pointnet2.py --train-area kitti_train --val-area kitti_val --cross-domain    # -> models/cross_domain/pointnet2_kitti_train.ckpt
    python train_pointnet2.py --features xyz --epochs 20 --ckpt out/pointnet2.ckpt

The options are ``train_pointnet.py``'s, with ``--features`` in place of ``--arch``: 'rgb' is what the script builds today (:178: the
colour is l0_points, 6 and 131 input channels at layer1 and fa_layer4), 'xyz' the network of the shipped pointnet2_model5 index
(:177: 3 and 128).  ``--mode`` only names the output (:308-311).  Staging, the per-batch choice of 1024 of a cell's 2048 rows, jitter
and the epoch loop are ``train_pointnet.py``'s own functions: the reference runs the same host code for both modes.  DESIGN.md §3.14.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import train_pointnet as host      # noqa: E402


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--mode', default='pointnet2', help='names the output only: models/<mode>_model<val>.ckpt')
    ap.add_argument('--train-area', default='1,2,3,4,6')
    ap.add_argument('--val-area', default='5')
    ap.add_argument('--cross-domain', action='store_true')
    ap.add_argument('--data-dir', default='data')
    ap.add_argument('--model-dir', default='models')
    ap.add_argument('--ckpt', default=None, help='output checkpoint prefix (default: the reference naming scheme)')
    ap.add_argument('--features', default='rgb', choices=('rgb', 'xyz'))
    ap.add_argument('--batch-size', type=int, default=100)
    ap.add_argument('--epochs', type=int, default=50)
    ap.add_argument('--val-step', type=int, default=10)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--device', default='cuda:0')
    return ap.parse_args(argv)


def main(argv=None):
    args = parse(argv)

    def make_trainer(classes):
        from learn_region_grow_amd.pointnet2_train import PointNet2Trainer
        return PointNet2Trainer(args.batch_size, classes, rgb_features=args.features == 'rgb', device=args.device)
    return host.run(args, make_trainer, 'train_pointnet2.py')


if __name__ == '__main__':
    sys.exit(main())
