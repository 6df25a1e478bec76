#!/usr/bin/env python3
"""Command-line driver with the job of the reference's ``animate_region_growing.py``: ONE room grown step by step on the GPU, two
pictures per step -- ``<out>/step%03d.png`` (current set green, neighbour set blue, the five text lines of :397-401) and
``<out>/seg%03d.png`` (every point in the colour of the region that last held it) -- and the per-region lines of :310.

    python animate_region_growing.py --area 5 --room 44                  # data/s3dis_area5.h5 + models/lrgnet_model5.ckpt -> tmp/
    python animate_region_growing.py --h5 rooms.h5 --room 0 --synthetic-weights --size 512 --max-frames 40 --out frames/
    python animate_region_growing.py --area 5 --orbit 0.01               # the camera rotation the reference has commented out (:377-381)

No OpenGL, GLUT, PIL or font file: the room's raw points are rasterised once on the GPU into a visibility buffer, every frame is a
look-up through it (learn_region_grow_amd.render), the text comes from a bitmap font of the package, and the frames are written as
palette PNGs.  The growth itself is the counter stream's lock-step packed iteration, one step per host call, followed on the device by
learn_region_grow_amd.trace.GrowthTrace: greedy growing only (no restarts, no beam), and not ``--rng legacy``.
"""
import argparse
import os
import sys
import time

import numpy as np

from region_grow import CLASSES_S3DIS, region_lines


def _triple(text):
    v = [float(x) for x in text.split(',')]
    if len(v) != 3:
        raise argparse.ArgumentTypeError('three comma-separated numbers expected, got %r' % text)
    return tuple(v)


def parse(argv=None):
    from learn_region_grow_amd import render
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--area', default='5', help="S3DIS area number, 'scannet', ... (the reference's AREA, :32)")
    ap.add_argument('--room', type=int, default=44, help='index of the room in the file (ROOM, :33)')
    ap.add_argument('--h5', default=None, help='room file (overrides --area for the data)')
    ap.add_argument('--ckpt', default=None, help='checkpoint prefix (default models/lrgnet_model<area>.ckpt, :265)')
    ap.add_argument('--synthetic-weights', action='store_true', help='seeded random weights instead of a checkpoint')
    ap.add_argument('--data-dir', default='data')
    ap.add_argument('--model-dir', default='models')
    ap.add_argument('--out', default='tmp', help='directory of the pictures (:402,:409)')
    ap.add_argument('--size', type=int, default=1000, help='width and height of the pictures (:238)')
    ap.add_argument('--point-size', type=int, default=5, help='glPointSize (:171): an odd number of pixels')
    ap.add_argument('--camera', type=_triple, default=render.CAMERA, help='eye X,Y,Z (:43-45)')
    ap.add_argument('--look-at', type=_triple, default=render.LOOK_AT, help='centre X,Y,Z (:46-48)')
    ap.add_argument('--orbit', type=float, default=0.0, help='radians the eye turns about z per step (:377-381); 0 = one fixed camera')
    ap.add_argument('--every', type=int, default=1, help='draw every N-th step only')
    ap.add_argument('--max-frames', type=int, default=0, help='stop after this many drawn steps (0 = the whole room)')
    ap.add_argument('--frames-per-batch', type=int, default=16, help='steps between two synchronisations with the GPU')
    ap.add_argument('--policy', default='net', choices=['net', 'gt', 'threshold'])
    ap.add_argument('--rng', default='counter', choices=['counter', 'legacy'])
    ap.add_argument('--resolution', type=float, default=0.1)
    ap.add_argument('--preprocess', default='gpu-exact', choices=['gpu-exact', 'host'])
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--device', default='cuda:0')
    args = ap.parse_args(argv)
    if args.rng == 'legacy':
        ap.error("--rng legacy is not traced: its nine-launch step ends behind the mask update and leaves a different state on the device; "
                 "the trace follows the counter stream's packed iteration")
    if args.point_size < 1 or args.point_size % 2 == 0:
        ap.error('--point-size must be odd: a point is a square centred on its pixel')
    if args.size < 8 or args.every < 1 or args.frames_per_batch < 1 or args.max_frames < 0:
        ap.error('--size >= 8, --every >= 1, --frames-per-batch >= 1 and --max-frames >= 0 expected')
    return args


def run(args):
    """-> dict(steps, pictures, seconds of the grow-and-draw loop, lines): the job of the script for parsed arguments."""
    import torch
    from learn_region_grow_amd import checkpoint, preprocess, preprocess_gpu, render, synthetic, trace
    from learn_region_grow_amd import io as lio
    from learn_region_grow_amd.lrgnet import LrgNetHIP

    if not torch.cuda.is_available():
        raise SystemExit('animate_region_growing.py needs a GPU (the HIP path has no CPU fallback)')
    device = torch.device(args.device)
    torch.cuda.set_device(device)
    if args.synthetic_weights:
        weights = synthetic.make_synthetic_weights(seed=args.seed, feature_size=13, lite=0)
        print('Synthetic weights (seed %d)' % args.seed)
    else:
        mp = args.ckpt or os.path.join(args.model_dir, 'lrgnet_model%s.ckpt' % args.area)
        weights = checkpoint.load_lrgnet_weights(mp, feature_size=13, lite=None)
        print('Restored network from %s' % mp)                                                # :267
    path = args.h5 or os.path.join(args.data_dir, ('%s.h5' if not str(args.area).isdigit() else 's3dis_area%s.h5') % args.area)
    all_points, all_obj_id, all_cls_id = lio.loadFromH5(path)
    if not 0 <= args.room < len(all_points):
        raise SystemExit('%s holds %d rooms: no room %d' % (path, len(all_points), args.room))
    raw, obj_raw, cls_raw = all_points[args.room], all_obj_id[args.room], all_cls_id[args.room]
    if args.preprocess == 'host':
        pre = preprocess.preprocess_room(raw, obj_raw, cls_raw, resolution=args.resolution)
    else:
        pre = preprocess_gpu.preprocess_room(raw, obj_raw, cls_raw, resolution=args.resolution, device=device, eig='exact')
    print('points', pre['points'].shape)                                                      # :163
    room = dict(points=pre['points'], obj_id=pre['obj_id'], order=pre['order'].astype(np.int32), room_id=args.room)
    n = len(room['points'])
    net = LrgNetHIP(1, 1, 512, 512, 13, None, device=device).load_weights(weights)
    grower = trace.make_grower(net, seed=args.seed, policy=args.policy, resolution=args.resolution)
    tr = trace.GrowthTrace(grower, room, pre['unequalized_idx'], frames_per_batch=args.frames_per_batch)
    rd = render.Renderer(raw[:, :3], pre['unequalized_idx'], n, args.size, args.size, args.point_size, device=device)
    rd.build_visibility(args.camera, args.look_at)
    os.makedirs(args.out, exist_ok=True)
    pal = rd.palette
    img_id, steps, t0, stop = 0, 0, time.time(), False
    for batch in tr.batches():
        keep = [k for k in range(len(batch)) if (batch.first + k) % args.every == 0]
        if args.max_frames:
            keep = keep[:max(0, args.max_frames - img_id)]
        steps = batch.first + len(batch)
        if keep:
            sel = torch.tensor(keep, dtype=torch.int64, device=device)
            index = torch.cat([batch.codes.index_select(0, sel), batch.paints.index_select(0, sel)])
            texts = [render.text_lines(*[int(x) for x in batch.headers[k][[1, 3, 4, 5, 6]]]) for k in keep]
            if args.orbit:
                frames = []
                for j, k in enumerate(keep):           # a camera of its own per step: the eye after (step index + 1) turns
                    rd.build_visibility(render.orbit_eye(args.camera, args.orbit * (batch.first + k + 1)), args.look_at)
                    frames.append(rd.shade(index[[j, len(keep) + j]].contiguous(), [render.LUT_STEP, render.LUT_SEG], [texts[j], None]))
                step_px = torch.stack([f[0] for f in frames]).cpu().numpy()
                seg_px = torch.stack([f[1] for f in frames]).cpu().numpy()
            else:
                px = rd.shade(index, [render.LUT_STEP] * len(keep) + [render.LUT_SEG] * len(keep), texts + [None] * len(keep)).cpu().numpy()
                step_px, seg_px = px[:len(keep)], px[len(keep):]
            for j in range(len(keep)):
                lio.write_png(os.path.join(args.out, 'step%03d.png' % img_id), step_px[j], pal)   # :402
                lio.write_png(os.path.join(args.out, 'seg%03d.png' % img_id), seg_px[j], pal)     # :409
                img_id += 1
        if args.max_frames and img_id >= args.max_frames:
            stop = True
            break
    dt = time.time() - t0
    if stop:
        torch.cuda.synchronize(device)
        res = grower.collect(fill=False)[0]            # the regions committed so far
    else:
        res = tr.result(fill=False)
    classes = None if 'kitti' in str(args.area) or args.area == 'scannet' else CLASSES_S3DIS
    lines = region_lines(args.room, res, pre['obj_id'], pre['cls_id'], classes)
    for ln in lines:
        print(ln)
    print('%d steps traced, %d pictures of %d x %d in %s: %.2f s (%.1f steps/s)' % (steps, 2 * img_id, args.size, args.size, args.out, dt, steps / max(dt, 1e-9)))
    return dict(steps=steps, pictures=2 * img_id, seconds=dt, lines=lines)


def main(argv=None):
    run(parse(argv))
    return 0


if __name__ == '__main__':
    sys.exit(main())
