#!/usr/bin/env python3
"""Command-line driver with the job of the reference's ``train_pointnet.py --mode pointnet``: the rooms of ``data/s3dis_area<k>.h5``
(or ``data/<area>.h5`` for 's3dis', 'scannet', 'kitti_train', 'kitti_val') cut into cells of 2048 rows (:327-350), the plain
PointNet trained on the GPU with the reference's loss, batch norm, learning-rate schedule and Adam (:63-111), the reference's epoch
lines, and the weights saved as a TensorFlow checkpoint bundle that ``pointnet.py --ckpt`` (and the reference's ``Saver.restore``)
reads.

    python train_pointnet.py --train-area 1,2,3,4,6 --val-area 5              # -> models/pointnet_model5.ckpt
    python train_pointnet.py --train-area kitti_train --val-area kitti_val --cross-domain
    python train_pointnet.py --arch shipped --epochs 20 --ckpt out/pointnet.ckpt

Options of the reference that are kept: --mode, --train-area, --val-area, --cross-domain.  ``--mode pointnet2`` is refused: training
PointNet++ needs the gradients of the whole sampling and interpolation stack and has a driver of its own, ``train_pointnet2.py``.  ``--arch`` picks
the network: 'today' is what the script builds now ((64,64,64,128,1024) / (512,256)), 'shipped' the one of the shipped
pointnet_model5 ((64,64,128,512) / (512,)).  Staging, the per-batch choice of 1024 of a cell's 2048 rows (:399-402) and jitter_data
(:235-246) make the legacy NumPy generator's draws in the script's order, seeded by --seed.  The last partial batch is dropped (:388).
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

AREAS = ['1', '2', '3', '4', '5', '6', 's3dis', 'scannet', 'kitti_train', 'kitti_val']           # :320, in this order
NUM_CLASSES = {'kitti': 260, 'scannet': 41}                                                      # class_util.py: classes_kitti, classes_nyu40; else classes_s3dis (13)


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--mode', default='pointnet')
    ap.add_argument('--train-area', default='1,2,3,4,6')
    ap.add_argument('--val-area', default='5')
    ap.add_argument('--cross-domain', action='store_true')
    ap.add_argument('--data-dir', default='data')
    ap.add_argument('--model-dir', default='models')
    ap.add_argument('--ckpt', default=None, help='output checkpoint prefix (default: the reference naming scheme)')
    ap.add_argument('--arch', default='today', choices=('today', 'shipped'))
    ap.add_argument('--batch-size', type=int, default=100)
    ap.add_argument('--epochs', type=int, default=50)
    ap.add_argument('--val-step', type=int, default=10)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--device', default='cuda:0')
    return ap.parse_args(argv)


def model_path(args):
    """:308-311."""
    if args.ckpt:
        return args.ckpt
    if args.cross_domain:
        return os.path.join(args.model_dir, 'cross_domain', '%s_%s.ckpt' % (args.mode, args.train_area.split(',')[0]))
    return os.path.join(args.model_dir, '%s_model%s.ckpt' % (args.mode, args.val_area.split(',')[0]))


def num_classes(train_area):
    """:312."""
    first = train_area.split(',')[0]
    for key, n in NUM_CLASSES.items():
        if key in first:
            return n
    return 13


def area_file(args, area):
    """:323-326."""
    return os.path.join(args.data_dir, '%s.h5' % area if area in AREAS[6:] else 's3dis_area%s.h5' % area)


def stage(args, rs):
    """:316-355: the cells of every room of the training and validation areas."""
    from learn_region_grow_amd import io
    from learn_region_grow_amd.pointnet_train import stage_cells
    train_areas, val_areas = args.train_area.split(','), args.val_area.split(',')
    parts = dict(train_points=[], train_labels=[], val_points=[], val_labels=[])
    for area in AREAS:
        if area not in train_areas and area not in val_areas:
            continue
        rooms, _, cls_ids = io.loadFromH5(area_file(args, area))
        for room_id in range(len(rooms)):
            pts, lab = stage_cells(rooms[room_id], cls_ids[room_id], area, rs)
            print('room_id %d/%d grid %d' % (room_id, len(rooms), len(pts)))
            for which, areas in (('val', val_areas), ('train', train_areas)):
                if area in areas:
                    parts[which + '_points'].extend(pts)
                    parts[which + '_labels'].extend(lab)
    return {k: np.array(v) for k, v in parts.items()}


def run_epoch(trainer, points, labels, rs, batch_size, train):
    """:388-410 / :415-435: mean loss and accuracy over the whole batches."""
    from learn_region_grow_amd.pointnet_train import NUM_POINT, jitter
    input_points = np.zeros((batch_size, NUM_POINT, 6))
    input_labels = np.zeros((batch_size, NUM_POINT))
    rows = []
    for b in range(int(len(labels) / batch_size)):
        start = b * batch_size
        if points.shape[1] == NUM_POINT:
            input_points[:] = points[start:start + batch_size]
            input_labels = labels[start:start + batch_size]
        else:
            for i in range(batch_size):
                subset = rs.choice(points.shape[1], NUM_POINT, replace=False)
                input_points[i] = points[start + i, subset]
                input_labels[i] = labels[start + i, subset]
        if train:
            sc = trainer.train_step(jitter(input_points, rs), input_labels)
        else:
            sc = trainer.evaluate(input_points, input_labels)
        rows.append((sc['loss'], sc['acc']))
    return np.mean(np.array(rows, dtype=np.float64), axis=0) if rows else np.array([np.nan, np.nan])


def run(args, make_trainer, script):
    """Everything after the arguments are parsed, for this driver and train_pointnet2.py: make_trainer(classes) builds the trainer once
    the cells are staged; script is the driver's name in the message of a machine without a GPU."""
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('%s needs a GPU (the HIP path has no CPU fallback)' % script)
    out = model_path(args)
    classes = num_classes(args.train_area)
    print('train', args.train_area.split(','), 'val', args.val_area.split(','), 'model', out, 'classes', classes)
    rs = np.random.RandomState(args.seed)
    data = stage(args, rs)
    for name, key in (('Train', 'train'), ('Validation', 'val')):
        lab = data[key + '_labels']
        print('%s Points' % name, data[key + '_points'].shape)
        print('%s Labels' % name, lab.shape, *((lab.min(), lab.max()) if lab.size else ()))
    if len(data['train_labels']) < args.batch_size:
        raise SystemExit('%d training cells are fewer than one batch of %d: nothing trained, no checkpoint written'
                         % (len(data['train_labels']), args.batch_size))
    trainer = make_trainer(classes).init_weights(args.seed)
    for epoch in range(args.epochs):
        idx = np.arange(len(data['train_labels']))
        rs.shuffle(idx)                                                                   # :380-383
        loss, acc = run_epoch(trainer, data['train_points'][idx], data['train_labels'][idx], rs, args.batch_size, True)
        print('Epoch: %d Loss: %.3f (cls %.3f)' % (epoch, loss, acc))                     # :411
        if epoch % args.val_step == args.val_step - 1 and len(data['val_labels']) >= args.batch_size:
            loss, acc = run_epoch(trainer, data['val_points'], data['val_labels'], rs, args.batch_size, False)
            print('Validation: %d Loss: %.3f (cls %.3f)' % (epoch, loss, acc))            # :436
    os.makedirs(os.path.dirname(out) or '.', exist_ok=True)
    trainer.save(out)
    print('Saved %s' % out)
    return 0


def main(argv=None):
    args = parse(argv)
    if args.mode == 'pointnet2':
        raise SystemExit('train_pointnet.py: --mode pointnet2 is not supported here: training PointNet++ needs the gradients of the whole '
                         'sampling and interpolation stack and has a driver of its own, train_pointnet2.py (DESIGN.md §7); use --mode pointnet')
    if args.mode != 'pointnet':
        raise SystemExit("train_pointnet.py: unknown --mode %r (only 'pointnet')" % args.mode)

    def make_trainer(classes):
        from learn_region_grow_amd.pointnet_train import ARCHITECTURES, PointNetTrainer
        conv, fc = ARCHITECTURES[args.arch]
        return PointNetTrainer(args.batch_size, conv, fc, classes, device=args.device)
    return run(args, make_trainer, 'train_pointnet.py')


if __name__ == '__main__':
    sys.exit(main())
