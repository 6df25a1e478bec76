#!/usr/bin/env python3
"""Command-line driver with the job of the reference's ``train_mcpnet.py``: stage the 512-point blocks of the S3DIS areas, train
MCPNet on the GPU with the semi-hard triplet loss, print the reference's epoch lines and save a TensorFlow checkpoint bundle that
``mcpnet.py --ckpt`` (and the reference's ``Saver.restore``) reads.

    python train_mcpnet.py --stage --areas 1,2,3,4,5,6     # the stage_data block (:70-150): data/s3dis_area%d.h5 -> data/mcp_area%d.h5
    python train_mcpnet.py --area 5                        # VAL_AREA (:152-155) -> models/mcpnet_model5.ckpt

The network is the one of the shipped mcpnet_model5.ckpt (feature_size 6: neighbor_pl = neighbor_points, input_pl = points), batches
of 256 with 16 samples an instance, Adam at 0.001, margin 1, 50 epochs, validation every 10th (:207).  ``--seed`` seeds the staging
draws (the script's numpy.random.seed(0)), the initial weights, the epoch shuffle (unseeded in the script) and even_sampling.
One RandomState runs through all rooms of all staged areas.  DESIGN.md §3.17.
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
    ap.add_argument('--stage', action='store_true', help='write data/mcp_area%%d.h5 for --areas and exit')
    ap.add_argument('--areas', default='1,2,3,4,5,6', help='the areas staged, or the areas loaded for training (:71, :168)')
    ap.add_argument('--area', type=int, default=1, help='VAL_AREA: held out, and names the checkpoint')
    ap.add_argument('--epochs', type=int, default=50)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--data', default='data', help='directory of s3dis_area%%d.h5 and mcp_area%%d.h5')
    ap.add_argument('--model', default=None, help='checkpoint prefix (default models/mcpnet_model<area>.ckpt)')
    ap.add_argument('--device', default=None, help='default: cuda:0')
    return ap.parse_args(argv)


def stage(args):
    from learn_region_grow_amd import io, mcpnet_train
    state = np.random.RandomState(args.seed)                 # :12, one stream through every room of every area
    for area in [int(a) for a in args.areas.split(',')]:
        points, obj_ids, _ = io.loadFromH5(os.path.join(args.data, 's3dis_area%d.h5' % area))
        staged = mcpnet_train.stage_area(list(zip(points, obj_ids)), state, area=area, device=args.device)
        mcpnet_train.write_staged(os.path.join(args.data, 'mcp_area%d.h5' % area), *staged)
    return 0


def run_epoch(trainer, points, rows, labels, order, state, train):
    """One pass over the blocks in `order` (:193-204, :213-224): the means of loss, acc, bg, wg and F over the batches."""
    from learn_region_grow_amd import mcpnet_train
    out = []
    for i in order:
        idx = mcpnet_train.even_sampling(labels[i], trainer.B, mcpnet_train.SAMPLES_PER_INSTANCE, state)
        if len(idx) != trainer.B:
            continue
        step = trainer.train_step if train else trainer.evaluate
        r = step(points[i][idx], rows[i][idx], labels[i][idx])
        out.append((r['loss'], mcpnet_train.nn_accuracy(r['emb'], labels[i][idx])) + mcpnet_train.anova(r['emb'], labels[i][idx]))
    with np.errstate(all='ignore'):
        return tuple(np.nanmean(np.array(out, dtype=np.float64), axis=0)) if out else (float('nan'),) * 5


def main(argv=None):
    args = parse(argv)
    if args.stage:
        return stage(args)
    from learn_region_grow_amd import mcpnet_train
    model = args.model or os.path.join('models', 'mcpnet_model%d.ckpt' % args.area)
    sets = {True: [], False: []}
    for area in [int(a) for a in args.areas.split(',')]:
        path = os.path.join(args.data, 'mcp_area%d.h5' % area)
        print('Loading %s ...' % path)
        sets[area == args.area].append(mcpnet_train.read_staged(path))
    train, val = ([np.concatenate([s[k] for s in sets[v]]) if sets[v] else np.zeros((0,)) for k in range(3)] for v in (False, True))
    if not len(train[0]):
        sys.exit('train_mcpnet.py: no training blocks (every area of --areas is the validation area)')
    print('train', len(train[1]), train[1][0].shape)
    print('val', len(val[1]), val[1][0].shape if len(val[1]) else ())
    trainer = mcpnet_train.MCPNetTrainer(mcpnet_train.BATCH_SIZE, device=args.device).init_weights(args.seed)
    state = np.random.RandomState(args.seed + 1)
    fmt = '%s %d loss %.2f acc %.2f bg %.2f wg %.2f F %.2f'
    for epoch in range(args.epochs):
        print(fmt % (('Epoch', epoch) + run_epoch(trainer, train[0], train[1], train[2], state.permutation(len(train[0])), state, True)))
        if epoch % 10 == 9 and len(val[0]):
            print(fmt % (('Validation', epoch) + run_epoch(trainer, val[0], val[1], val[2], state.permutation(len(val[0])), state, False)))
    if trainer.skipped_batches:
        print('%d batches without a positive pair were skipped' % trainer.skipped_batches)
    trainer.save(model)
    print('Saved %s' % model)
    return 0


if __name__ == '__main__':
    sys.exit(main())
