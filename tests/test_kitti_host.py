"""CPU: the KITTI staging's host side.  The twin (tests/kitti_ref.py) against the reference script's own output on the golden
sequence, the fixture's coverage of every rule, the chain arithmetic against the script's BLAS expressions, the set order of the original
ids, io.read_png, and the command line's flags, file pairing and lines."""
import os
import struct
import zlib

import numpy as np
import pytest

import kitti_fixture as kf
import kitti_ref
from learn_region_grow_amd import io as lio
from learn_region_grow_amd import kitti

import stage_semantic_kitti as cli


@pytest.mark.parametrize('k', [0, 1])
def test_twin_equals_reference_script(k):
    o = kf.load()['sets'][k]
    samples, lines, _ = kf.twin(k)
    assert len(samples) >= 2
    points = np.vstack([s['points'] for s in samples])
    assert points.dtype == np.float32 and points.tobytes() == o['points'].tobytes()
    assert [len(s['points']) for s in samples] == o['count_room'].tolist()
    assert lines == o['lines']


@pytest.mark.parametrize('k', [0, 1])
def test_fixture_reaches_every_rule(k):
    o = kf.load()['sets'][k]
    _, _, cover = kf.twin(k)
    print(cover)
    for name in ('invalid_from_map', 'invalid_refused_later', 'valid_black', 'moving', 'labelled_overwritten', 'linked_through_labelled',
                 'small_component', 'component_at_threshold', 'unlabelled_without_edge', 'unfinished_scans'):
        assert cover[name] > 0, name
    assert cover['original_ids'] >= 3                     # the fewest of any sample
    assert o['min_cluster'] >= 2
    assert 6 <= len(kf.load()['scans']) <= 9 and all(1200 <= len(s) <= 1500 for s in kf.load()['scans'])
    assert os.path.getsize(os.path.join(kf.GOLDEN, 'kitti_stage_small.npz')) < 400 * 1000


def test_chain_arithmetic_equals_blas_expressions():
    """The script's expressions (a BLAS product per scan) against the twin's chains: every float32 output coordinate, every voxel key at both
    resolutions, every pixel and every validity flag of the fixture."""
    seq = kf.load()
    poses = kitti_ref.transform_poses(seq['tr'], seq['raw_poses'])
    images = seq['images']
    pr = kitti_ref.project_stack(seq['scans'], seq['labels'], images, poses, seq['tr'], seq['p2'], seq['voxel_resolution'])
    ends = np.cumsum([len(s) for s in seq['scans']])
    for s, (a, b) in enumerate(zip(np.concatenate([[0], ends[:-1]]), ends)):
        local = seq['scans'][s][:, 0:3]
        world = local.dot(poses[s][:3, :3].T) + poses[s][:3, 3]
        assert np.array_equal(world.astype(np.float32), pr['xyz'][a:b].astype(np.float32))
        for res in (seq['voxel_resolution'], seq['downsample_resolution']):
            assert np.array_equal(np.round(world / res).astype(int), np.round(pr['xyz'][a:b] / res).astype(int))
        hom = np.hstack((local, np.ones(len(local)).reshape(-1, 1)))
        hom = seq['p2'].dot(seq['tr'].dot(hom.T)).T
        uv = np.round(hom[:, :2] / hom[:, 2:3]).astype(int)
        H, W = images[s].shape[:2]
        valid = (hom[:, 2] > 0) & (uv[:, 0] >= 0) & (uv[:, 0] < W) & (uv[:, 1] >= 0) & (uv[:, 1] < H)
        assert np.array_equal(valid, pr['valid'][a:b])
        assert 0 < valid.sum() < len(valid)


def test_original_ids_iterate_as_the_set_of_the_column():
    columns = [s['eq'][:, 6] for k in (0, 1) for s in kf.twin(k)[0]]
    rs = np.random.RandomState(3)
    for n_ids in (1, 5, 40, 700, 5000):                   # past several growths of the set's table
        ids = rs.choice(np.arange(1, 65536), n_ids, replace=False)
        columns.append(np.concatenate([[0.0], rs.choice(ids, 4 * n_ids), ids, [0.0]])[rs.permutation(5 * n_ids + 2)].astype(np.float64))
    columns.append(np.zeros(7))
    columns.append(np.array([3.0, 3.0, 3.0]))
    for col in columns:
        assert kitti.original_ids(col) == list(set(col) - set([0]))


@pytest.mark.parametrize('colour_type, shape', [(2, (19, 23, 3)), (6, (7, 5, 4)), (0, (11, 13))])
def test_read_png_every_filter_type(tmp_path, colour_type, shape):
    image = np.random.RandomState(colour_type).randint(0, 256, shape).astype(np.uint8)
    image[0:2] = 255                                      # sums that wrap
    path = str(tmp_path / 'a.png')
    kf.write_png(path, image, colour_type, filters=(0, 1, 2, 3, 4, 4, 3, 2, 1))
    want = np.repeat(image[:, :, None], 3, axis=2) if colour_type == 0 else image[:, :, :3]
    got = lio.read_png(path)
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
    for f in range(5):                                    # each filter type on every row, the first one included
        kf.write_png(path, image, colour_type, filters=(f,))
        assert np.array_equal(lio.read_png(path), want)


def test_read_png_against_pil(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    y, x = np.mgrid[0:40, 0:61]
    smooth = np.stack([(3 * x) % 256, (5 * y) % 256, (x + y) % 256], axis=2).astype(np.uint8)      # PIL chooses filters per row
    noise = np.random.RandomState(1).randint(0, 256, (33, 47, 3)).astype(np.uint8)
    for k, image in enumerate((smooth, noise, smooth[:, :, 0], np.dstack([noise, noise[:, :, :1]]))):
        path = str(tmp_path / ('%d.png' % k))
        Image.fromarray(image).save(path)
        assert np.array_equal(lio.read_png(path), np.asarray(Image.open(path).convert('RGB')))
        kf.write_png(path, image, {2: 0, 3: 2 if image.shape[-1] == 3 else 6}[image.ndim])
        assert np.array_equal(np.asarray(Image.open(path).convert('RGB')), lio.read_png(path))


def test_read_png_refuses_what_it_does_not_decode(tmp_path):
    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xFFFFFFFF)

    def png(depth=8, colour=2, interlace=0, raw=b'\x00' + b'\x01' * 6):
        return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', 2, 1, depth, colour, 0, 0, interlace)) + chunk(b'IDAT', zlib.compress(raw)) +
                chunk(b'IEND', b''))
    path = str(tmp_path / 'b.png')
    cases = dict(ok=png(), depth16=png(depth=16), palette=png(colour=3), grey_alpha=png(colour=4), interlaced=png(interlace=1),
                 short=png(raw=b'\x00\x01'), filter5=png(raw=b'\x05' + b'\x01' * 6), not_png=b'GIF89a' + b'\x00' * 20, truncated=png()[:40],
                 bad_crc=png()[:-5] + b'\x00' + png()[-4:])
    for name, data in cases.items():
        with open(path, 'wb') as f:
            f.write(data)
        if name == 'ok':
            assert lio.read_png(path).tolist() == [[[1, 1, 1], [1, 1, 1]]]
        else:
            with pytest.raises(ValueError):
                lio.read_png(path)


def test_flags_are_the_reference_scripts():
    a = cli.parse(['-d', 'D', '-o', 'O'])
    assert (a.dataset, a.output, a.sequences, a.interval, a.min_cluster, a.voxel_resolution, a.downsample_resolution, a.distance_span, a.skip) == \
        ('D', 'O', '00,01,02,03,04,05,06,07,08,09,10', 20, 50, 0.3, 0.1, 50.0, 10)
    a = cli.parse(['-d', 'D', '-o', 'O', '-s', '08', '-i', '3', '-m', '7', '-v', '0.25', '-r', '0.05', '-p', '9', '-k', '2', '--something-else', '1'])
    b = cli.parse(['--dataset', 'D', '--output', 'O', '--sequences', '08', '--interval', '3', '--min-cluster', '7', '--voxel-resolution', '0.25',
                   '--downsample-resolution', '0.05', '--distance-span', '9', '--skip', '2'])
    assert vars(a) == vars(b)
    assert (a.sequences, a.interval, a.min_cluster, a.voxel_resolution, a.downsample_resolution, a.distance_span, a.skip) == ('08', 3, 7, 0.25, 0.05, 9.0, 2)
    with pytest.raises(SystemExit):
        cli.parse(['-o', 'O'])


def test_files_are_parsed_and_paired_as_the_script_does(tmp_path):
    seq = kf.load()
    root = kf.write_dataset(tmp_path)
    base = os.path.join(root, 'sequences', '00')
    calib = kitti.read_calib(os.path.join(base, 'calib.txt'))
    assert sorted(calib) == ['P0', 'P2', 'Tr'] and np.array_equal(calib['Tr'], seq['tr']) and np.array_equal(calib['P2'], seq['p2'])
    poses = kitti.read_poses(os.path.join(base, 'poses.txt'), calib['Tr'])
    want = kitti_ref.transform_poses(seq['tr'], seq['raw_poses'])
    assert len(poses) == len(want) and all(p.tobytes() == w.tobytes() for p, w in zip(poses, want))
    scans, labels, images = kitti.list_sequence(root, '00')
    n = len(seq['scans'])
    assert [os.path.basename(p) for p in scans] == ['%06d.bin' % k for k in range(n)]
    assert [os.path.basename(p) for p in labels] == ['%06d.label' % k for k in range(n)]
    assert [os.path.basename(p) for p in images] == ['%06d.png' % k for k in range(n)]
    assert np.array_equal(lio.read_png(images[3]), seq['images'][3])
    os.rename(images[0], os.path.join(base, 'image_2', 'zz.png'))      # pairing is by position in the sorted lists, not by name
    assert [os.path.basename(p) for p in kitti.list_sequence(root, '00')[2]] == ['%06d.png' % k for k in range(1, n)] + ['zz.png']
    os.remove(labels[-1])
    with pytest.raises(ValueError):
        kitti.list_sequence(root, '00')


@pytest.mark.parametrize('k', [0, 1])
def test_sample_loop_lines_and_file(tmp_path, monkeypatch, capsys, k):
    """The command line's loop, lines and room file with the device calls replaced by the twin's: which scans form a sample, which are only
    counted, what is printed and what io.loadFromH5 reads back."""
    seq = kf.load()
    o = seq['sets'][k]
    root = kf.write_dataset(tmp_path / 'kitti')
    stacks = []

    def fuse(scans, labels, images, poses, tr, p2, vres, downsample_resolution, min_cluster, device, times):
        stacks.append(len(scans))
        r = kitti_ref.fuse_sample(scans, labels, images, poses, tr, p2, vres, downsample_resolution, min_cluster)
        return dict(points=r['points'], kept_per_scan=r['project']['kept_per_scan'], line=r['line'])

    def counts(scans, labels, images, poses, tr, p2, vres, device, times):
        stacks.append(-len(scans))
        return kitti_ref.project_stack(scans, labels, images, poses, tr, p2, vres)['kept_per_scan']
    monkeypatch.setattr(kitti, 'fuse_sample', fuse)
    monkeypatch.setattr(kitti, 'kept_counts', counts)
    out = str(tmp_path / 'out' / 'kitti_val.h5')
    cli.main(['-d', root, '-o', out, '-s', '00', '-i', str(o['interval']), '-k', str(o['skip']), '-m', str(o['min_cluster']),
              '-v', repr(seq['voxel_resolution']), '-r', repr(seq['downsample_resolution']), '-p', '12'])
    assert capsys.readouterr().out.splitlines() == o['lines']
    assert stacks == [o['interval']] * len(o['count_room']) + [-(len(seq['scans']) - max(kf.sample_offsets(len(seq['scans']), o['interval'], o['skip'])) -
                                                                 (o['skip'] + 1) * o['interval'])]
    rooms = lio.loadFromH5(out, load_labels=False)
    assert [len(r) for r in rooms] == o['count_room'].tolist()
    assert np.vstack(rooms).tobytes() == o['points'].tobytes()
    feats, obj, cls = lio.loadFromH5(out)
    assert feats[0].shape[1] == 6 and obj[0].min() >= 1 and cls[0].max() < 250
