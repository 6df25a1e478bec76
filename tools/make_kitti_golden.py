#!/usr/bin/env python
"""Makes tests/golden/kitti_stage_small.npz: a synthetic SemanticKITTI sequence and what the reference's stage_semantic_kitti.py itself
computes from it under two option sets (its `points`, `count_room` and printed lines).

    python tools/make_kitti_golden.py --reference /path/to/learn_region_grow [--out tests/golden/kitti_stage_small.npz]

The sequence is written to a temporary directory in the dataset's layout; the script is run in this process with runpy after stand-ins for
`imageio` (imread through PIL) and `h5py` (a File that keeps what create_dataset is given) are placed in sys.modules.  It needs PIL, yaml
and networkx, and is never run by a test.  The scene is built so that every rule of DESIGN 3.19 is reached; min_cluster of each option
set is chosen from the scene (tests/kitti_ref.py's counts) so that one component sits exactly at min_cluster + 1 nodes.
"""
import argparse
import contextlib
import io
import os
import runpy
import sys
import tempfile
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SCANS, W, H = 9, 96, 32
OPTION_SETS = [dict(interval=2, skip=1, at_least=2), dict(interval=4, skip=0, at_least=6)]          # min_cluster is chosen below, from at_least on
VOXEL, DOWN = 0.3, 0.1


def box(x0, y0, z0, nx, ny, nz, step=0.1):
    g = np.mgrid[0:nx, 0:ny, 0:nz].reshape(3, -1).T * step
    return g + np.array([x0, y0, z0])


def make_world(rs):
    """World points [n, 3] on the centres of 0.1 m cells (multiples of 0.1), with object and class ids."""
    parts = []

    def add(p, obj, cls):
        parts.append(np.hstack([p, np.full((len(p), 1), obj), np.full((len(p), 1), cls)]))
    for k, (x, y, obj) in enumerate([(6.0, 2.1, 1), (9.0, -2.4, 2), (3.0, -1.8, 3), (12.0, 1.5, 7)]):      # labelled cars
        add(box(x, y, -1.2, 9, 5, 3), obj, 10)
    add(box(3.9, -1.8, -1.2, 6, 5, 3), 0, 10)                  # unlabelled car points touching car 3
    # two unlabelled groups of class 50 joined only through the one labelled voxel between them (labelled points emit no edges)
    for k in range(7):
        add(box(7.2, -0.6 + 0.3 * k, -0.6, 1, 1, 2), 5 if k == 3 else 0, 50)
    for j in range(8):                                          # unlabelled lines of 3 .. 10 voxels, a class each
        for k in range(3 + j):
            add(box(2.4 + 0.3 * k, 3.0 - 0.9 * j + (0.0 if j < 4 else -0.3), 0.0, 2, 1, 1), 0, 70 + j)
    for j in range(6):                                          # unlabelled points on their own
        add(np.array([[4.5 + 1.5 * j, 0.6, 0.6]]), 0, 90 + j)
    add(box(5.1, 0.0, -1.2, 4, 4, 3), 9, 252)                   # a moving object
    g = np.mgrid[-40:170, -50:50].reshape(2, -1).T * 0.1        # ground, unlabelled
    g = g[rs.rand(len(g)) < 0.5]
    add(np.hstack([g, np.full((len(g), 1), -1.8)]), 0, 40)
    return np.vstack(parts)


def make_sequence(seed=7):
    rs = np.random.RandomState(seed)
    world = make_world(rs)
    special = world[:, 4] != 40
    tr = np.eye(4)
    tr[:3] = [[0.0, -1.0, 0.0, 0.02], [0.0, 0.0, -1.0, -0.07], [1.0, 0.0, 0.0, -0.25]]
    p2 = np.eye(4)
    p2[:3] = [[30.0, 0.0, 48.0, 1.5], [0.0, 30.0, 10.0, 0.2], [0.0, 0.0, 1.0, 0.003]]
    scans, labels, images, raw_poses = [], [], [], []
    for k in range(N_SCANS):
        yaw = 0.45 * np.sin(1.3 * k)
        lidar = np.eye(4)
        lidar[:3, :3] = [[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]]
        lidar[:3, 3] = [0.6 * k, 0.05 * k, 0.0]
        raw_poses.append(np.matmul(tr, np.matmul(lidar, np.linalg.inv(tr))))
        n = 1200 + int(rs.randint(0, 301))
        ground = np.nonzero(~special)[0]
        pick = np.concatenate([np.nonzero(special)[0], rs.choice(ground, n - int(special.sum()), replace=False)])
        pick = pick[rs.permutation(len(pick))]
        p = world[pick, :3] + np.where(special[pick, None], 0.0, rs.uniform(-0.03, 0.03, (len(pick), 3)) * [1.0, 1.0, 0.0])
        local = np.matmul(p - lidar[:3, 3], lidar[:3, :3])     # R^T (p - t)
        scan = np.zeros((n, 4), dtype=np.float32)
        scan[:, :3] = np.round(local * 256.0) / 256.0
        scans.append(scan)
        labels.append((world[pick, 3].astype(np.uint32) << 16) | world[pick, 4].astype(np.uint32))
        img = rs.randint(1, 256, (H, W, 3)).astype(np.uint8)
        img[10:22, 52:70] = 0
        images.append(img)
    return dict(scans=scans, labels=labels, images=images, raw_poses=raw_poses, tr=tr, p2=p2)


def write_dataset(root, seq, sequence='00'):
    from PIL import Image
    d = os.path.join(root, 'sequences', sequence)
    for sub in ('velodyne', 'labels', 'image_2'):
        os.makedirs(os.path.join(d, sub))
    with open(os.path.join(root, 'semantic-kitti.yaml'), 'w') as f:
        f.write('labels:\n  0: "unlabeled"\n')
    with open(os.path.join(d, 'calib.txt'), 'w') as f:
        for key, m in (('P0', seq['p2']), ('P2', seq['p2']), ('Tr', seq['tr'])):
            f.write('%s: %s\n' % (key, ' '.join(repr(float(v)) for v in m[:3].reshape(-1))))
    with open(os.path.join(d, 'poses.txt'), 'w') as f:
        for m in seq['raw_poses']:
            f.write(' '.join(repr(float(v)) for v in m[:3].reshape(-1)) + '\n')
    for k in range(len(seq['scans'])):
        seq['scans'][k].tofile(os.path.join(d, 'velodyne', '%06d.bin' % k))
        seq['labels'][k].tofile(os.path.join(d, 'labels', '%06d.label' % k))
        Image.fromarray(seq['images'][k]).save(os.path.join(d, 'image_2', '%06d.png' % k))


def run_reference(script, dataset, opts):
    """The reference script in this process; returns (points float32, count_room int32, printed lines)."""
    from PIL import Image
    kept = {}

    class File(object):
        def __init__(self, name, mode):
            pass

        def create_dataset(self, name, data=None, dtype=None, **kw):
            kept[name] = np.array(data, dtype=dtype)

        def close(self):
            pass
    stand_ins = {'imageio': types.ModuleType('imageio'), 'h5py': types.ModuleType('h5py')}
    stand_ins['imageio'].imread = lambda path: np.asarray(Image.open(path))
    stand_ins['h5py'].File = File
    saved_argv, saved_mods = sys.argv, {k: sys.modules.get(k) for k in stand_ins}
    sys.modules.update(stand_ins)
    sys.argv = [script, '-d', dataset, '-o', os.path.join(dataset, 'out.h5'), '-s', '00', '-i', str(opts['interval']), '-k', str(opts['skip']),
                '-m', str(opts['min_cluster']), '-v', repr(VOXEL), '-r', repr(DOWN)]
    out = io.StringIO()
    try:
        with contextlib.redirect_stdout(out):
            runpy.run_path(script, run_name='__main__')
    finally:
        sys.argv = saved_argv
        for k, m in saved_mods.items():
            if m is None:
                del sys.modules[k]
            else:
                sys.modules[k] = m
    return kept['points'].reshape(-1, 8), kept['count_room'], out.getvalue().splitlines()


def choose_min_cluster(seq, opts):
    """The smallest min_cluster >= at_least under which the twin reaches every rule (one component exactly at min_cluster + 1 nodes)."""
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    import kitti_ref
    names = ['/sequences/00/velodyne/%06d.bin' % k for k in range(N_SCANS)]
    for m in range(opts['at_least'], 24):
        _, _, cover = kitti_ref.stage_sequence(seq['scans'], seq['labels'], seq['images'], names, seq['raw_poses'], seq['tr'], seq['p2'],
                                               opts['interval'], opts['skip'], m, VOXEL, DOWN)
        missing = [k for k, v in cover.items() if v == 0 or (k == 'original_ids' and v < 3)]
        print('interval %d skip %d min_cluster %d: %s' % (opts['interval'], opts['skip'], m, cover))
        if not missing:
            return m
    raise SystemExit('no min_cluster reaches every rule: change the scene')


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reference', required=True, help="the reference's checkout (holds stage_semantic_kitti.py)")
    ap.add_argument('--out', default=os.path.join(REPO, 'tests', 'golden', 'kitti_stage_small.npz'))
    args = ap.parse_args()
    seq = make_sequence()
    out = dict(tr=seq['tr'], p2=seq['p2'], raw_poses=np.array(seq['raw_poses']), scan_counts=np.array([len(s) for s in seq['scans']], dtype=np.int32),
               scans=np.vstack(seq['scans']), labels=np.concatenate(seq['labels']), images=np.array(seq['images']),
               voxel_resolution=np.float64(VOXEL), downsample_resolution=np.float64(DOWN))
    with tempfile.TemporaryDirectory() as tmp:
        write_dataset(tmp, seq)
        for k, opts in enumerate(OPTION_SETS):
            opts = dict(interval=opts['interval'], skip=opts['skip'], min_cluster=choose_min_cluster(seq, opts))
            points, count, lines = run_reference(os.path.join(args.reference, 'stage_semantic_kitti.py'), tmp, opts)
            out['options_%d' % k] = np.array([opts['interval'], opts['skip'], opts['min_cluster']], dtype=np.int32)
            out['points_%d' % k], out['count_room_%d' % k], out['lines_%d' % k] = points, count, np.array(lines)
            print('option set %d: %s, %d rows in %d samples' % (k, opts, len(points), len(count)))
    np.savez_compressed(args.out, **out)
    print('%s: %d bytes' % (args.out, os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
