#!/usr/bin/env python
"""One sample of stage_semantic_kitti.py at the dataset's own shape: 20 scans of about 120 k points with 1241x376 camera images, generated
in a temporary directory in the dataset's layout.  Writes profiles/kitti_stage_bench.json.

Measured: the kernels by device events (lrg_kitti_project, lrg_kitti_first_in_voxel at both resolutions, lrg_kitti_components), the sample end
to end through kitti.stage_sequences by the host clock -- file reads and PNG decoding split out -- warmed and repeated, and the host twin
of the tests (tests/kitti_ref.py: dicts and plain Python loops, the shape of the reference script's own loops) once on the same sample, for
scale.  The twin's rows are compared with the device's.

    python tools/kitti_stage_bench.py [--scans 20] [--points 120000] [--repeats 3] [--no-twin] [--out profiles/kitti_stage_bench.json]
"""
import argparse
import json
import os
import struct
import sys
import tempfile
import time
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
W, H = 1241, 376


def spread(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)), runs=[float(x) for x in xs])


def write_png(path, image):
    """RGB PNG whose rows cycle through the five filter types, as an encoder with adaptive filtering would mix them."""
    h, w = image.shape[:2]
    cur = image.reshape(h, w * 3).astype(np.int32)
    up = np.vstack([np.zeros((1, w * 3), np.int32), cur[:-1]])
    left = np.hstack([np.zeros((h, 3), np.int32), cur[:, :-3]])
    upleft = np.hstack([np.zeros((h, 3), np.int32), up[:, :-3]])
    p = left + up - upleft
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - upleft)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
    preds = [np.zeros_like(cur), left, up, (left + up) // 2, paeth]
    kind = np.arange(h) % 5
    body = np.zeros((h, w * 3), np.int32)
    for f in range(5):
        body[kind == f] = (cur - preds[f])[kind == f]
    raw = np.hstack([kind.reshape(-1, 1).astype(np.uint8), (body & 255).astype(np.uint8)]).tobytes()

    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xFFFFFFFF)
    with open(path, 'wb') as f:
        f.write(b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)) + chunk(b'IDAT', zlib.compress(raw, 1)) + chunk(b'IEND', b''))


def make_dataset(root, n_scans, n_points, seed=5):
    """A street: ground, two rows of facades, parked cars with instance ids, a few moving points; the vehicle drives 1 m a scan."""
    rs = np.random.RandomState(seed)
    d = os.path.join(root, 'sequences', '00')
    for sub in ('velodyne', 'labels', 'image_2'):
        os.makedirs(os.path.join(d, sub))
    tr = np.array([[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, -0.08], [1.0, 0.0, 0.0, -0.27]])
    p2 = np.array([[718.856, 0.0, 607.1928, 45.38225], [0.0, 718.856, 185.2157, -0.1130887], [0.0, 0.0, 1.0, 0.003779761]])
    tr4 = np.vstack([tr, [0.0, 0.0, 0.0, 1.0]])
    with open(os.path.join(d, 'calib.txt'), 'w') as f:
        for key, m in (('P0', p2), ('P1', p2), ('P2', p2), ('P3', p2), ('Tr', tr)):
            f.write('%s: %s\n' % (key, ' '.join(repr(float(v)) for v in m.reshape(-1))))
    cars = rs.uniform([-30.0, -7.0], [60.0, 7.0], (40, 2))
    cars[:, 1] = np.where(cars[:, 1] > 0, 5.5, -5.5)
    with open(os.path.join(d, 'poses.txt'), 'w') as pf:
        for k in range(n_scans):
            yaw = 0.01 * k
            lidar = np.eye(4)
            lidar[:3, :3] = [[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]]
            lidar[:3, 3] = [1.0 * k, 0.02 * k, 0.0]
            pose = np.matmul(tr4, np.matmul(lidar, np.linalg.inv(tr4)))
            pf.write(' '.join(repr(float(v)) for v in pose[:3].reshape(-1)) + '\n')
            n = n_points + int(rs.randint(-4000, 4001))
            kind = rs.choice(4, n, p=[0.62, 0.28, 0.09, 0.01])
            r, a = 45.0 * np.sqrt(rs.rand(n)), rs.uniform(0, 2 * np.pi, n)
            world = np.stack([lidar[0, 3] + r * np.cos(a), lidar[1, 3] + r * np.sin(a), -1.73 + rs.normal(0, 0.02, n)], axis=1)
            wall = kind == 1
            world[wall, 1] = np.where(rs.rand(int(wall.sum())) < 0.5, 9.0, -9.0) + rs.normal(0, 0.03, int(wall.sum()))
            world[wall, 2] = rs.uniform(-1.7, 6.0, int(wall.sum()))
            car = kind >= 2
            which = rs.randint(0, len(cars), n)
            world[car, :2] = cars[which[car]] + rs.uniform([-2.0, -0.9], [2.0, 0.9], (int(car.sum()), 2))
            world[car, 2] = rs.uniform(-1.6, -0.2, int(car.sum()))
            cls = np.choose(kind, [40, 50, 10, 252]).astype(np.uint32)
            obj = np.where(car & (which % 4 != 0), which + 1, 0).astype(np.uint32)          # every fourth car carries no instance id
            scan = np.zeros((n, 4), dtype=np.float32)
            scan[:, :3] = np.matmul(world - lidar[:3, 3], lidar[:3, :3])
            scan.tofile(os.path.join(d, 'velodyne', '%06d.bin' % k))
            ((obj << 16) | cls).tofile(os.path.join(d, 'labels', '%06d.label' % k))
            y, x = np.mgrid[0:H, 0:W]
            image = np.stack([(x // 3 + 7 * k) % 255 + 1, (y + 3 * k) % 255 + 1, ((x + y) // 2) % 255 + 1], axis=2).astype(np.uint8)
            image[rs.randint(0, H, 4000), rs.randint(0, W, 4000)] = 0
            write_png(os.path.join(d, 'image_2', '%06d.png' % k), image)
    return root


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--scans', type=int, default=20)
    ap.add_argument('--points', type=int, default=120000)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--no-twin', action='store_true')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'kitti_stage_bench.json'))
    args = ap.parse_args(argv)
    import torch
    from learn_region_grow_amd import kitti
    if not torch.cuda.is_available():
        raise SystemExit('kitti_stage_bench.py needs a GPU: a timing taken without one says nothing')
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        make_dataset(tmp, args.scans, args.points)
        print('dataset generated in %.1f s' % (time.perf_counter() - t0), flush=True)
        opts = dict(interval=args.scans, skip=0, min_cluster=50, voxel_resolution=0.3, downsample_resolution=0.1)
        lines = []
        rooms = kitti.stage_sequences(tmp, ['00'], log=lines.append, **opts)                                   # warm-up: code object, allocator
        wall, parts = [], []
        for _ in range(args.repeats):
            times = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            again = kitti.stage_sequences(tmp, ['00'], log=lambda s: None, times=times, **opts)
            wall.append(time.perf_counter() - t0)
            parts.append(times)
            assert again[0].tobytes() == rooms[0].tobytes()
        names = sorted(parts[0])
        res = dict(workload='one sample: %d scans of about %d points, %dx%d images; -i %d -m 50 -v 0.3 -r 0.1' % (args.scans, args.points, W, H, args.scans),
                   device=torch.cuda.get_device_name(0), line=lines[-1], rows=int(len(rooms[0])),
                   sample_wall_s=spread(wall), parts_ms={n: spread([p[n] for p in parts]) for n in names},
                   device_and_host_glue_s=spread([w - 1e-3 * (p['read_ms'] + p['png_ms']) for w, p in zip(wall, parts)]),
                   note='sample_wall_s: kitti.stage_sequences end to end by the host clock; read_ms (scan and label files) and png_ms (io.read_png) are host '
                        'times inside it; project_ms, downsample_ms, equalize_ms and components_ms are device events around each call; '
                        'device_and_host_glue_s = wall less reads and PNG decoding (uploads, the kernels, torch compactions, the download)')
        if not args.no_twin:
            import kitti_ref
            calib = kitti.read_calib(os.path.join(tmp, 'sequences', '00', 'calib.txt'))
            scan_names, label_names, image_names = kitti.list_sequence(tmp, '00')
            scans, labels, images = kitti._read_stack(scan_names, label_names, image_names, range(args.scans))
            poses = kitti.read_poses(os.path.join(tmp, 'sequences', '00', 'poses.txt'), calib['Tr'])
            t0 = time.perf_counter()
            want = kitti_ref.fuse_sample(scans, labels, images, poses[:args.scans], calib['Tr'], calib['P2'], 0.3, 0.1, 50)
            res['twin'] = dict(path='tests/kitti_ref.fuse_sample (dicts and Python loops), the same sample, files already read, one run',
                               wall_s=time.perf_counter() - t0, equals_device=bool(want['points'].tobytes() == rooms[0].tobytes()), line=want['line'])
            res['twin_over_device_glue'] = res['twin']['wall_s'] / res['device_and_host_glue_s']['median']
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
