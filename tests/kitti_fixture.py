"""The golden KITTI sequence (tests/golden/kitti_stage_small.npz, made by tools/make_kitti_golden.py) for the host and the GPU tests: its
arrays, the dataset directory the command line reads, a PNG writer that uses every filter type, and the twin's results, computed once."""
import os
import struct
import zlib

import numpy as np

from conftest import GOLDEN

import kitti_ref

_cache = {}


def load():
    """dict: scans / labels / images per scan, raw_poses, tr, p2, the two resolutions and per option set (interval, skip, min_cluster),
    the reference script's points, count_room and lines."""
    if 'seq' not in _cache:
        z = np.load(os.path.join(GOLDEN, 'kitti_stage_small.npz'))
        ends = np.cumsum(z['scan_counts'])
        seq = dict(scans=np.split(z['scans'], ends[:-1]), labels=np.split(z['labels'], ends[:-1]), images=list(z['images']),
                   raw_poses=list(z['raw_poses']), tr=z['tr'], p2=z['p2'], voxel_resolution=float(z['voxel_resolution']),
                   downsample_resolution=float(z['downsample_resolution']), sets=[])
        seq['names'] = ['/sequences/00/velodyne/%06d.bin' % k for k in range(len(seq['scans']))]
        for k in range(2):
            interval, skip, min_cluster = (int(v) for v in z['options_%d' % k])
            seq['sets'].append(dict(interval=interval, skip=skip, min_cluster=min_cluster, points=z['points_%d' % k],
                                    count_room=z['count_room_%d' % k], lines=[str(s) for s in z['lines_%d' % k]]))
        _cache['seq'] = seq
    return _cache['seq']


def twin(k):
    """kitti_ref.stage_sequence on option set k: (samples, lines, cover), computed once and not to be changed."""
    if ('twin', k) not in _cache:
        seq = load()
        o = seq['sets'][k]
        _cache['twin', k] = kitti_ref.stage_sequence(seq['scans'], seq['labels'], seq['images'], seq['names'], seq['raw_poses'], seq['tr'], seq['p2'],
                                                     o['interval'], o['skip'], o['min_cluster'], seq['voxel_resolution'], seq['downsample_resolution'])
    return _cache['twin', k]


def sample_offsets(n_scans, interval, skip):
    return list(range(0, n_scans - interval + 1, (skip + 1) * interval))


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def write_png(path, image, colour_type=2, filters=(0, 1, 2, 3, 4)):
    """8-bit non-interlaced PNG of image [H, W] (colour_type 0) or [H, W, 3 or 4] (2 or 6); row r is filtered with filters[r % len]."""
    image = np.asarray(image, dtype=np.uint8)
    H, W = image.shape[:2]
    bpp = {0: 1, 2: 3, 6: 4}[colour_type]
    rows = image.reshape(H, W * bpp).astype(int)
    raw = bytearray()
    for r in range(H):
        f = filters[r % len(filters)]
        cur, up = rows[r], rows[r - 1] if r else np.zeros(W * bpp, dtype=int)
        out = []
        for i in range(W * bpp):
            a = cur[i - bpp] if i >= bpp else 0
            c = up[i - bpp] if i >= bpp else 0
            pred = (0, a, up[i], (a + up[i]) // 2, paeth(a, up[i], c))[f]
            out.append((cur[i] - pred) & 255)
        raw.append(f)
        raw.extend(out)

    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xFFFFFFFF)
    data = zlib.compress(bytes(raw))
    half = len(data) // 2                                # two IDAT chunks: a decoder has to join them
    with open(path, 'wb') as f:
        f.write(b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, colour_type, 0, 0, 0)) + chunk(b'tEXt', b'Comment\x00test') +
                chunk(b'IDAT', data[:half]) + chunk(b'IDAT', data[half:]) + chunk(b'IEND', b''))


def write_dataset(root, seq=None, sequence='00', with_yaml=False):
    """The dataset layout the command line reads: sequences/<sequence>/{calib.txt, poses.txt, velodyne/, labels/, image_2/}."""
    seq = seq or load()
    d = os.path.join(str(root), 'sequences', sequence)
    for sub in ('velodyne', 'labels', 'image_2'):
        os.makedirs(os.path.join(d, sub))
    if with_yaml:
        with open(os.path.join(str(root), 'semantic-kitti.yaml'), 'w') as f:
            f.write('labels:\n  0: "unlabeled"\n')
    with open(os.path.join(d, 'calib.txt'), 'w') as f:
        for key, m in (('P0', seq['p2']), ('P2', seq['p2']), ('Tr', seq['tr'])):
            f.write('%s: %s\n' % (key, ' '.join(repr(float(v)) for v in np.asarray(m)[:3].reshape(-1))))
    with open(os.path.join(d, 'poses.txt'), 'w') as f:
        for m in seq['raw_poses']:
            f.write(' '.join(repr(float(v)) for v in np.asarray(m)[:3].reshape(-1)) + '\n')
    for k in range(len(seq['scans'])):
        np.asarray(seq['scans'][k], dtype=np.float32).tofile(os.path.join(d, 'velodyne', '%06d.bin' % k))
        np.asarray(seq['labels'][k], dtype=np.uint32).tofile(os.path.join(d, 'labels', '%06d.label' % k))
        write_png(os.path.join(d, 'image_2', '%06d.png' % k), seq['images'][k])
    return str(root)
