"""GPU: the KITTI staging kernels (csrc/lrg_kitti.hip) and learn_region_grow_amd.kitti against the reference script's golden output and the
host twin (tests/kitti_ref.py).  Every comparison is exact."""
import numpy as np
import pytest

import kitti_fixture as kf
import kitti_ref
from learn_region_grow_amd import _lib
from learn_region_grow_amd import io as lio
from learn_region_grow_amd import kitti

import stage_semantic_kitti as cli

pytestmark = pytest.mark.gpu


def stack_args(seq, which):
    poses = kitti_ref.transform_poses(seq['tr'], seq['raw_poses'])
    return ([seq['scans'][i] for i in which], [seq['labels'][i] for i in which], [seq['images'][i] for i in which], [poses[i] for i in which],
            seq['tr'], seq['p2'], seq['voxel_resolution'])


def fuse_all(seq, o, device):
    out = []
    for start in kf.sample_offsets(len(seq['scans']), o['interval'], o['skip']):
        out.append(kitti.fuse_sample(*stack_args(seq, range(start, start + o['interval'])), downsample_resolution=seq['downsample_resolution'],
                                     min_cluster=o['min_cluster'], device=device))
    return out


@pytest.mark.parametrize('k', [0, 1])
def test_fuse_sample_equals_reference_script(cuda_device, k):
    seq = kf.load()
    o = seq['sets'][k]
    first, second = fuse_all(seq, o, cuda_device), fuse_all(seq, o, cuda_device)
    points = np.vstack([r['points'] for r in first])
    assert points.dtype == np.float32 and points.tobytes() == o['points'].tobytes()
    assert [len(r['points']) for r in first] == o['count_room'].tolist()
    assert [r['line'] for r in first] == [l for l in o['lines'] if l.startswith('Creating')]
    assert np.vstack([r['points'] for r in second]).tobytes() == points.tobytes()          # the same bytes every time


@pytest.mark.parametrize('k', [0, 1])
def test_command_line_equals_reference_script(cuda_device, tmp_path, capsys, k):
    seq = kf.load()
    o = seq['sets'][k]
    root = kf.write_dataset(tmp_path / 'kitti')
    out = str(tmp_path / 'kitti_val.h5')
    cli.main(['-d', root, '-o', out, '-s', '00', '-i', str(o['interval']), '-k', str(o['skip']), '-m', str(o['min_cluster']),
              '-v', repr(seq['voxel_resolution']), '-r', repr(seq['downsample_resolution']), '--device', str(cuda_device)])
    assert capsys.readouterr().out.splitlines() == o['lines']
    rooms = lio.loadFromH5(out, load_labels=False)
    assert [len(r) for r in rooms] == o['count_room'].tolist()
    assert np.vstack(rooms).dtype == np.float32 and np.vstack(rooms).tobytes() == o['points'].tobytes()


def check_kernels_against_twin(args, downsample_resolution, device):
    """Each kernel alone on the twin's own intermediates."""
    import torch
    scans, labels, images, poses, tr, p2, vres = args
    want = kitti_ref.fuse_sample(scans, labels, images, poses, tr, p2, vres, downsample_resolution, 5)
    pr, wp = kitti.project_stack(*args, device=device), want['project']
    assert pr['xyz'].cpu().numpy().tobytes() == wp['xyz'].tobytes()                        # float64 chains, bit for bit
    assert np.array_equal(pr['valid'].cpu().numpy(), wp['valid'])
    assert np.array_equal(pr['rgb'].cpu().numpy(), wp['rgb'])
    assert np.array_equal(pr['keep'].cpu().numpy(), wp['keep'])
    assert np.array_equal(pr['obj'].cpu().numpy(), wp['obj']) and np.array_equal(pr['cls'].cpu().numpy(), wp['cls'])
    assert kitti.kept_counts(*args, device=device) == wp['kept_per_scan']
    kept = wp['xyz'][wp['keep']]
    rep = kitti.first_in_voxel(torch.from_numpy(kept).to(device), downsample_resolution, device=device).cpu().numpy()
    assert np.array_equal(rep, want['rep_ds'])
    ds = kept[want['rep_ds'] == np.arange(len(kept))]
    rep = kitti.first_in_voxel(torch.from_numpy(ds).to(device), vres, device=device).cpu().numpy()
    assert np.array_equal(rep, want['rep_eq'])
    eq, wc = want['eq'], want['comp']
    comp = kitti.components(torch.from_numpy(np.ascontiguousarray(eq[:, :3])).to(device), torch.from_numpy(eq[:, 6].astype(np.int32)).to(device),
                            torch.from_numpy(eq[:, 7].astype(np.int32)).to(device), vres, device=device)
    root = comp['root'].cpu().numpy()
    assert np.array_equal(root, wc['root'])
    assert np.array_equal(comp['emits'].cpu().numpy(), wc['emits'])
    at_root = root == np.arange(len(root))
    assert np.array_equal(comp['size'].cpu().numpy()[at_root], wc['size'][at_root])
    assert np.array_equal(comp['first_src'].cpu().numpy()[at_root], wc['first_src'][at_root])
    return want


def test_each_kernel_against_the_twin(cuda_device):
    seq = kf.load()
    want = check_kernels_against_twin(stack_args(seq, range(0, 4)), seq['downsample_resolution'], cuda_device)
    assert (want['comp']['size'] > 1).sum() > 5 and want['comp']['emits'].sum() > 100


def larger_sample():
    """3 scans of 20 011 points: no multiple of a block, several block-sum tiles, a table of 2^17 slots with long probe runs (many
    points share few cells), voxels shared within and across scans, labelled and unlabelled points of three classes."""
    seq = kf.load()
    rs = np.random.RandomState(11)
    n, n_scans = 20011, 3
    sites = np.round(rs.uniform([1.0, -9.0, -1.9], [22.0, 9.0, 0.4], (6000, 3)) * 20.0) / 20.0
    site_cls = np.where(sites[:, 2] < -1.5, 40, np.where(sites[:, 1] > 0, 10, 50))
    site_obj = np.where((site_cls == 10) & (rs.rand(len(sites)) < 0.7), 1 + (sites[:, 0] // 4).astype(int), 0)
    site_obj = np.where((site_cls == 50) & (rs.rand(len(sites)) < 0.1), 30, site_obj)
    scans, labels, images, poses = [], [], [], []
    for s in range(n_scans):
        yaw = 0.3 * s - 0.3
        pose = np.eye(4)
        pose[:3, :3] = [[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]]
        pose[:3, 3] = [1.1 * s, -0.2 * s, 0.01 * s]
        pick = rs.randint(0, len(sites), n)
        world = sites[pick] + rs.uniform(-0.12, 0.12, (n, 3))
        scan = np.zeros((n, 4), dtype=np.float32)
        scan[:, :3] = np.matmul(world - pose[:3, 3], pose[:3, :3])
        scans.append(scan)
        cls = np.where(rs.rand(n) < 0.01, 253, site_cls[pick])
        labels.append(((site_obj[pick].astype(np.uint32)) << 16) | cls.astype(np.uint32))
        image = rs.randint(1, 256, (32, 96, 3)).astype(np.uint8)
        image[8:20, 40:60] = 0
        images.append(image)
        poses.append(pose)
    return scans, labels, images, poses, seq['tr'], seq['p2'], 0.3


def test_larger_sample_against_the_twin(cuda_device):
    args = larger_sample()
    want = check_kernels_against_twin(args, 0.1, cuda_device)
    cover = want['cover']
    print(cover, want['line'])
    assert cover['invalid_from_map'] > 100 and cover['invalid_refused_later'] > 10 and cover['valid_black'] > 100 and cover['moving'] > 100
    assert want['n_equalized'] > 10000 and want['n_downsampled'] > 2 * want['n_equalized']
    for min_cluster in (5, 60):
        w = kitti_ref.fuse_sample(*args, downsample_resolution=0.1, min_cluster=min_cluster) if min_cluster != 5 else want
        got = kitti.fuse_sample(*args, downsample_resolution=0.1, min_cluster=min_cluster, device=cuda_device)
        assert got['points'].tobytes() == w['points'].tobytes()
        assert got['line'] == w['line'] and got['kept_per_scan'] == w['project']['kept_per_scan']
        assert (got['n_downsampled'], got['n_equalized'], got['n_original'], got['n_labels']) == \
            (w['n_downsampled'], w['n_equalized'], w['n_original'], w['n_labels'])


@pytest.mark.parametrize('bad', [4.0e5, -4.0e5, float('nan'), float('inf')])
def test_coordinate_outside_the_key_window_raises(cuda_device, bad):
    import torch
    seq = kf.load()
    args = stack_args(seq, range(0, 2))
    scans = [s.copy() for s in args[0]]
    scans[1][77, 1] = bad                                  # 4e5 m / 0.3 m is past 2^20 cells
    with pytest.raises(_lib.LrgHipError):
        kitti.fuse_sample(scans, *args[1:], downsample_resolution=seq['downsample_resolution'], min_cluster=3, device=cuda_device)
    xyz = torch.zeros((300, 3), dtype=torch.float64, device=cuda_device)
    xyz[123, 2] = bad
    with pytest.raises(_lib.LrgHipError):
        kitti.first_in_voxel(xyz, 0.3, device=cuda_device)
    with pytest.raises(_lib.LrgHipError):
        kitti.components(xyz, torch.zeros(300, dtype=torch.int32, device=cuda_device), torch.zeros(300, dtype=torch.int32, device=cuda_device), 0.3,
                         device=cuda_device)
    # the last cell a key may name is 2^20 - 2 either way (its neighbours are probed): one cell further is refused
    edge = torch.zeros((2, 3), dtype=torch.float64, device=cuda_device)
    edge[1, 0] = float(2 ** 20 - 2)
    assert kitti.first_in_voxel(edge, 1.0, device=cuda_device).tolist() == [0, 1]
    edge[1, 0] = float(2 ** 20 - 1)
    with pytest.raises(_lib.LrgHipError):
        kitti.first_in_voxel(edge, 1.0, device=cuda_device)
