#!/usr/bin/env python3
"""Command-line driver with the job of the reference's ``train_region_grow.py``: staged tuples from ``data/staged_*.h5``
(written by ``stage_data.py`` or by ``learn_region_grow_amd.stage``), LrgNet trained on the GPU with the reference's losses
and Adam (learn_region_grow_util.py:165-189), the reference's epoch lines, weights saved as a TensorFlow checkpoint bundle
that ``region_grow.py`` (and the reference's ``Saver.restore``) reads.

    python train_region_grow.py --train-area 1,2,3,4,6 --val-area 5            # data/multiseed/seed<e % 8>_area<k>.h5 (training areas, one seed
                                                                               # per epoch), data/staged_area5.h5 (validation) -> models/lrgnet_model5.ckpt
    python train_region_grow.py --multiseed 0 --train-area 1,2,3,4,6           # data/staged_area<k>.h5
    python train_region_grow.py --staged my_tuples.h5 --ckpt out/lrgnet.ckpt --epochs 20
    python train_region_grow.py --assemble device --train-area 1,2,3,4,6       # the same files, uploaded once per load; batches drawn on the GPU
    python train_region_grow.py --stage online --train-area 1,2,3,4,6 --val-area 5   # from data/s3dis_area<k>.h5: no staged files at all

Options of the reference that are kept: --train-area, --val-area, --lite, --multiseed (data/multiseed/seed<k>_area<a>.h5, one seed
per epoch, train_region_grow.py:69-76), --cross-domain.  Batch assembly (pad / subsample each tuple to 512 + 512 points with the
legacy NumPy generator seeded 0) follows train_region_grow.py:156-175 call for call.

--assemble device (a build extension): the loaded tuples go to the GPU once (train_data.TupleStore), every batch is
drawn there under the counter stream keyed by (--seed, tuple id) at (epoch, pass), and the host synchronises once per epoch, to read the
epoch's statistics.  The epoch order is still the legacy generator's shuffle.  --stage online: no staged files; each epoch the training
areas' room files (stage_data.py's input names) go through stage.seed_transform(epoch % multiseed), preprocess_gpu.preprocess_rooms and the
device teacher with that seed and stay on the device; the validation area is staged once, unseeded.  Device memory grows with the areas:
roughly 4.6 GB per 68 rooms, transiently twice that while the areas are joined (an estimate; unmeasured at S3DIS scale).
"""
import argparse
import os
import sys
import time

import numpy as np


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--train-area', default='1,2,3,4,6')
    ap.add_argument('--val-area', default=None)
    ap.add_argument('--staged', default=None, help='comma list of staged files (overrides the area naming scheme)')
    ap.add_argument('--data-dir', default='data')
    ap.add_argument('--model-dir', default='models')
    ap.add_argument('--ckpt', default=None, help='output checkpoint prefix (default: the reference naming scheme)')
    ap.add_argument('--cross-domain', action='store_true')
    ap.add_argument('--multiseed', type=int, default=8, help='seeds cycled per epoch, data/multiseed/seed<k>_area<a>.h5 (reference default 8; 0 = data/staged_area<a>.h5)')
    ap.add_argument('--lite', type=int, default=None)
    ap.add_argument('--feature-size', type=int, default=13, choices=[6, 9, 12, 13])
    ap.add_argument('--batch-size', type=int, default=100)
    ap.add_argument('--epochs', type=int, default=50)
    ap.add_argument('--val-step', type=int, default=7)
    ap.add_argument('--learning-rate', type=float, default=1e-3)
    ap.add_argument('--init', default=None, help='checkpoint prefix to start from (default: the reference initialiser)')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--assemble', default=None, choices=['host', 'device'],
                    help="where a batch is put together: 'host' (default; the legacy generator, the reference's bits) or 'device' (counter stream, no upload per step)")
    ap.add_argument('--stage', default='files', choices=['files', 'online'],
                    help="'files' (default): staged files as stage_data.py writes them; 'online': stage the room files on the GPU every epoch (implies --assemble device)")
    ap.add_argument('--resolution', type=float, default=0.1, help='--stage online: the teacher\'s voxel size (stage_data.py --resolution)')
    ap.add_argument('--max-points', type=int, default=1024, help='--stage online: points per side of a tuple (stage_data.py --max-points)')
    args = ap.parse_args(argv)
    if args.stage == 'online':
        if args.assemble == 'host':
            ap.error('--stage online leaves the tuples on the device: it cannot go with --assemble host')
        if args.staged:
            ap.error('--stage online reads room files, not --staged files')
        args.assemble = 'device'
    elif args.assemble is None:
        args.assemble = 'host'
    return args


def model_path(args):
    """train_region_grow.py:37-53."""
    if args.ckpt:
        return args.ckpt
    val = args.val_area.split(',')[0] if args.val_area else 'None'
    d = args.model_dir
    if args.cross_domain:
        return os.path.join(d, 'cross_domain', 'lrgnet_%s.ckpt' % args.train_area.split(',')[0])
    suffix = {6: '_xyz', 9: '_xyzrgb', 12: '_xyzrgbn'}.get(args.feature_size, '')
    if not suffix and args.lite is not None:
        suffix = '_lite_%d' % args.lite
    return os.path.join(d, 'lrgnet_model%s%s.ckpt' % (val, suffix))


def staged_path(args, area, epoch, is_train=True):
    """train_region_grow.py:69-78: the multiseed files are for the TRAINING areas only (`elif MULTISEED > 0 and AREA in TRAIN_AREA`);
    a validation area always reads data/staged_area<a>.h5."""
    if str(area).startswith('synthetic'):
        return os.path.join(args.data_dir, 'staged_%s.h5' % area)
    if args.multiseed > 0 and is_train:
        return os.path.join(args.data_dir, 'multiseed', 'seed%d_area%s.h5' % (epoch % args.multiseed, area))
    return os.path.join(args.data_dir, 'staged_area%s.h5' % area)


def run_epoch(trainer, data, rs, batch_size, train=True, shuffle=True):
    """One pass over the tuples in batches (train_region_grow.py:141-183 / :186-219): mean loss and add / remove precision, recall."""
    from learn_region_grow_amd.stage import assemble_batch
    idx = np.arange(len(data['points']))
    if shuffle:
        rs.shuffle(idx)
    rows = []
    for b in range(len(idx) // batch_size):
        xi, xn, ia, ir = assemble_batch(data, idx[b * batch_size:(b + 1) * batch_size], rs, batch_size, trainer.Ni, trainer.Nn)
        if train:
            rows.append(trainer.train_step(xi, xn, ia, ir))
        else:
            sc = trainer.evaluate(xi, xn, ia, ir)              # forward + loss only (no dW / dX products)
            rows.append((sc['loss'], sc['add_prc'], sc['add_rcl'], sc['remove_prc'], sc['remove_rcl']))
    return np.mean(np.array(rows, dtype=np.float64), axis=0) if rows else np.zeros(5)


def run_epoch_device(trainer, store, rs, batch_size, epoch, bufs, train=True, shuffle=True):
    """run_epoch with the batches drawn on the device (train_data.TupleStore.assemble): the order is uploaded once, every step is launches
    only, and the one synchronisation is the read of the epoch's statistics, from which the same five means are taken."""
    import torch
    from learn_region_grow_amd.train_data import PASS_TRAIN, PASS_VALIDATION
    idx = np.arange(len(store))
    if shuffle:
        rs.shuffle(idx)
    steps = len(idx) // batch_size
    if not steps:
        return np.zeros(5)
    order = store.upload_order(idx)
    stats = torch.zeros((steps, 2, 8), dtype=torch.float64, device=trainer.dev)
    for b in range(steps):
        store.assemble(order[b * batch_size:(b + 1) * batch_size], epoch, PASS_TRAIN if train else PASS_VALIDATION, bufs)
        step = trainer.train_step_device if train else trainer.evaluate_device
        step(bufs.inlier, bufs.neighbor, bufs.add, bufs.remove, bufs.positives_remove, stats[b])
    rows = []
    for s in stats.cpu().numpy():
        sc = trainer._scalars(s)
        rows.append((sc['loss'], sc['add_prc'], sc['add_rcl'], sc['remove_prc'], sc['remove_rcl']))
    return np.mean(np.array(rows, dtype=np.float64), axis=0)


def stage_online(args, areas, seed, rooms_of):
    """The tuples of `areas` staged on the device as `stage_data.py --area <a> [--seed <seed>] --rng counter` would write them, area by area
    (the teacher's 2^31-row limit is per call), and left there: a TupleStore.  rooms_of caches the room files' contents between epochs."""
    import stage_data
    from learn_region_grow_amd import io as lio
    from learn_region_grow_amd import preprocess_gpu, stage
    from learn_region_grow_amd.train_data import TupleStore
    stores = []
    for area in areas:
        path = stage_data.input_path(argparse.Namespace(h5=None, data_dir=args.data_dir, seed=seed), area)
        if path not in rooms_of:
            if not os.path.exists(path):
                print('warning: room file %s does not exist' % path, file=sys.stderr)
                continue
            print('Loading %s ...' % path)
            rooms_of[path] = lio.loadFromH5(path)
        all_points, all_obj_id, all_cls_id = rooms_of[path]
        raw = [(stage.seed_transform(all_points[r], seed), all_obj_id[r], all_cls_id[r]) for r in range(len(all_points))]
        pre = preprocess_gpu.preprocess_rooms(raw, resolution=args.resolution, eig='exact', device=args.device) if raw else []
        rooms = [dict(points=p['points'], obj_id=p['obj_id'], room_id=r) for r, p in enumerate(pre)]
        staged = stage.stage_rooms_gpu(rooms, seed=seed or 0, resolution=args.resolution, max_points=args.max_points, device=args.device, download=False)
        stores.append(TupleStore.from_device(staged['device'], args.feature_size, rng_seed=args.seed))
    return TupleStore.concat(stores) if stores else None


def main(argv=None):
    args = parse(argv)
    if args.assemble == 'device':
        return main_device(args)
    import torch
    from learn_region_grow_amd import checkpoint, stage, synthetic
    from learn_region_grow_amd.train import LrgNetTrainer
    if not torch.cuda.is_available():
        raise SystemExit('train_region_grow.py needs a GPU (the HIP path has no CPU fallback)')
    torch.cuda.set_device(torch.device(args.device))
    rs = np.random.RandomState(args.seed)                                         # numpy.random.seed(0), train_region_grow.py:17
    trainer = LrgNetTrainer(args.batch_size, 512, 512, args.feature_size, args.lite, device=args.device, learning_rate=args.learning_rate)
    if args.init:
        trainer.load_weights(checkpoint.load_lrgnet_weights(args.init, feature_size=args.feature_size, lite=args.lite))
    else:
        trainer.load_weights(synthetic.make_reference_init_weights(seed=args.seed, feature_size=args.feature_size, lite=args.lite or 0))
    train_areas = args.train_area.split(',')
    val_areas = args.val_area.split(',') if args.val_area else []
    loaded, data, val = None, None, None
    epoch_time = []
    for epoch in range(args.epochs):
        files = args.staged.split(',') if args.staged else [staged_path(args, a, epoch) for a in train_areas]
        if loaded != files:                                                      # reloaded per epoch only under --multiseed (:60)
            parts = []
            for f in files:
                if os.path.exists(f):
                    print('Loading %s ...' % f)
                    parts.append(stage.load_staged(f, args.feature_size))
            if not parts:
                # (the reference skips a missing multiseed file, :75-76, and would then fail on an empty training set)
                print('warning: epoch %d: none of %s exists -- nothing to train on' % (epoch, ', '.join(files)), file=sys.stderr)
                continue
            data = {k: [x for p in parts for x in p[k]] for k in ('points', 'remove', 'neighbor_points', 'add')}
            loaded = files
            print('train', len(data['points']), data['points'][0].shape, len(data['neighbor_points']))
        t0 = time.time()
        ls, ap, ar, rp, rr = run_epoch(trainer, data, rs, args.batch_size)
        epoch_time.append(time.time() - t0)
        print('Epoch %d loss %.2f add %.2f/%.2f rmv %.2f/%.2f' % (epoch, ls, ap, ar, rp, rr))          # :183
        if val_areas and epoch % args.val_step == args.val_step - 1:                                   # :185-219
            if val is None:
                vfiles = [staged_path(args, a, 0, is_train=False) for a in val_areas]
                for f in vfiles:
                    if not os.path.exists(f):
                        print('warning: validation file %s does not exist' % f, file=sys.stderr)
                vparts = [stage.load_staged(f, args.feature_size) for f in vfiles if os.path.exists(f)]
                val = {k: [x for p in vparts for x in p[k]] for k in ('points', 'remove', 'neighbor_points', 'add')} if vparts else None
            if val:
                ls, ap, ar, rp, rr = run_epoch(trainer, val, rs, args.batch_size, train=False, shuffle=False)
                print('Validation %d loss %.2f add %.2f/%.2f rmv %.2f/%.2f' % (epoch, ls, ap, ar, rp, rr))
    if not epoch_time:
        raise SystemExit('no staged training file was found in any epoch (looked for e.g. %s): nothing trained, no checkpoint written'
                         % (args.staged or staged_path(args, train_areas[0], 0)))
    print('Avg Epoch Time: %.3f' % np.mean(epoch_time))
    out = model_path(args)
    os.makedirs(os.path.dirname(out) or '.', exist_ok=True)
    checkpoint.write_bundle(out, trainer.checkpoint_numpy())      # variables + Adam slots + beta powers + global step (99 entries)
    print('Saved %s' % out)
    return 0


def main_device(args):
    """main under --assemble device: the same epochs, lines and checkpoint, the tuples in a TupleStore."""
    import torch
    from learn_region_grow_amd import checkpoint, stage, synthetic
    from learn_region_grow_amd.train import LrgNetTrainer
    from learn_region_grow_amd.train_data import BatchBuffers, TupleStore
    if not torch.cuda.is_available():
        raise SystemExit('train_region_grow.py needs a GPU (the HIP path has no CPU fallback)')
    torch.cuda.set_device(torch.device(args.device))
    rs = np.random.RandomState(args.seed)
    trainer = LrgNetTrainer(args.batch_size, 512, 512, args.feature_size, args.lite, device=args.device, learning_rate=args.learning_rate)
    if args.init:
        trainer.load_weights(checkpoint.load_lrgnet_weights(args.init, feature_size=args.feature_size, lite=args.lite))
    else:
        trainer.load_weights(synthetic.make_reference_init_weights(seed=args.seed, feature_size=args.feature_size, lite=args.lite or 0))
    bufs = BatchBuffers(args.batch_size, trainer.Ni, trainer.Nn, args.feature_size, args.device)
    train_areas = args.train_area.split(',')
    val_areas = args.val_area.split(',') if args.val_area else []
    online = args.stage == 'online'
    rooms_of = {}

    def from_files(files):
        parts = []
        for f in files:
            if os.path.exists(f):
                print('Loading %s ...' % f)
                parts.append(stage.load_staged(f, args.feature_size))
        if not parts:
            return None
        data = {k: [x for p in parts for x in p[k]] for k in ('points', 'remove', 'neighbor_points', 'add')}
        return TupleStore.from_staged(data, args.feature_size, args.device, rng_seed=args.seed)
    loaded, store, val, val_tried = None, None, None, False
    epoch_time = []
    for epoch in range(args.epochs):
        if online:
            what = ('online', epoch % args.multiseed if args.multiseed > 0 else None)
        else:
            what = args.staged.split(',') if args.staged else [staged_path(args, a, epoch) for a in train_areas]
        if loaded != what:                                                       # restaged / reloaded per epoch only under --multiseed
            store = None                                                         # the old tuples go before the new ones come
            store = stage_online(args, train_areas, what[1], rooms_of) if online else from_files(what)
            if store is None or not len(store):
                print('warning: epoch %d: nothing to train on (%s)' % (epoch, 'no room file of the training areas' if online else ', '.join(what)), file=sys.stderr)
                store = None
                continue
            loaded = what
            print('train', len(store), (int(store.count_in[0]), store.F), len(store))
        t0 = time.time()
        ls, ap, ar, rp, rr = run_epoch_device(trainer, store, rs, args.batch_size, epoch, bufs)
        epoch_time.append(time.time() - t0)
        print('Epoch %d loss %.2f add %.2f/%.2f rmv %.2f/%.2f' % (epoch, ls, ap, ar, rp, rr))
        if val_areas and epoch % args.val_step == args.val_step - 1:
            if not val_tried:
                val_tried = True
                if online:
                    val = stage_online(args, val_areas, None, rooms_of)
                else:
                    vfiles = [staged_path(args, a, 0, is_train=False) for a in val_areas]
                    for f in vfiles:
                        if not os.path.exists(f):
                            print('warning: validation file %s does not exist' % f, file=sys.stderr)
                    val = from_files(vfiles)
            if val is not None and len(val):
                ls, ap, ar, rp, rr = run_epoch_device(trainer, val, rs, args.batch_size, epoch, bufs, train=False, shuffle=False)
                print('Validation %d loss %.2f add %.2f/%.2f rmv %.2f/%.2f' % (epoch, ls, ap, ar, rp, rr))
    if not epoch_time:
        raise SystemExit('nothing to train on was found in any epoch: nothing trained, no checkpoint written')
    print('Avg Epoch Time: %.3f' % np.mean(epoch_time))
    out = model_path(args)
    os.makedirs(os.path.dirname(out) or '.', exist_ok=True)
    checkpoint.write_bundle(out, trainer.checkpoint_numpy())
    print('Saved %s' % out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
