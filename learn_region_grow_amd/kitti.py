"""SemanticKITTI scans fused into scenes on the GPU -- the reference's ``stage_semantic_kitti.py``.

``read_calib`` / ``read_poses`` / ``list_sequence``   the files of one sequence, parsed and paired as the script does
``project_stack``    steps 2-5 for a stack of scans: lrg_kitti_project
``fuse_sample``      steps 1-10 for one sample (a full stack of ``interval`` scans)
``stage_sequences``  the sample loop over sequences; returns the rooms ``io.saveToH5`` takes

The kernels are csrc/lrg_kitti.hip.  Poses (a 4x4 product per scan) and the order of the original object ids (Python's set order) stay on
the host; compactions and the numbering of the qualifying components are ordered torch operations on the device (nonzero, cumsum).
There is no host path: without the library or a GPU the calls raise."""
import ctypes
import os

import numpy as np

from . import _lib

STATUS_TEXT = {_lib.LRG_KITTI_ST_NONFINITE: 'a coordinate is not finite', _lib.LRG_KITTI_ST_WINDOW: 'a voxel lies outside the 21-bit key window',
               _lib.LRG_KITTI_ST_SCAN: 'a scan index is out of range', _lib.LRG_KITTI_ST_TABLE: 'the voxel table is full'}


def _matrix(values):
    m = np.zeros((4, 4))
    m[:3] = np.asarray(values[:12], dtype=np.float64).reshape(3, 4)
    m[3, 3] = 1.0
    return m


def read_calib(path):
    """calib.txt: every ``key: 12 numbers`` line as a 4x4 matrix with the last row 0 0 0 1 (stage_semantic_kitti.py:43-54)."""
    calib = {}
    with open(path) as f:
        for line in f:
            key, content = line.strip().split(':')
            calib[key] = _matrix([float(v) for v in content.strip().split()])
    return calib


def read_poses(path, tr):
    """poses.txt: Tr^-1 pose Tr per line, in NumPy on the host (stage_semantic_kitti.py:57-69)."""
    tr_inv = np.linalg.inv(tr)
    with open(path) as f:
        return [np.matmul(tr_inv, np.matmul(_matrix([float(v) for v in line.strip().split()]), tr)) for line in f]


def _walk_sorted(top):
    return sorted(os.path.join(dp, f) for dp, dn, fn in os.walk(os.path.expanduser(top)) for f in fn)


def list_sequence(dataset, sequence):
    """(scans, labels, images): the sorted files under velodyne/, labels/ and image_2/ of a sequence, paired by position as the script pairs
    them.  Raises when there are fewer label or image files than scans."""
    base = os.path.join(dataset, 'sequences', sequence)
    scans, labels, images = (_walk_sorted(os.path.join(base, sub)) for sub in ('velodyne', 'labels', 'image_2'))
    if len(labels) < len(scans) or len(images) < len(scans):
        raise ValueError('sequence %s: %d scans but %d label files and %d images' % (sequence, len(scans), len(labels), len(images)))
    return scans, labels, images


def _status(d_status, what):
    st = int(d_status.item())
    if st:
        raise _lib.LrgHipError('%s: %s' % (what, '; '.join(t for b, t in sorted(STATUS_TEXT.items()) if st & b)))


class _Dev(object):
    """The device, its stream and the ctypes spelling of tensors."""

    def __init__(self, device):
        import torch
        self.torch = torch
        self.lib = _lib.load()
        self.dev = torch.device(device)
        torch.cuda.set_device(self.dev)
        self.st = ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    @staticmethod
    def ptr(t):
        return ctypes.c_void_p(t.data_ptr())

    def table(self, n):
        slots = self.lib.lrg_kitti_table_slots(int(n))
        if slots <= 0:
            raise _lib.LrgHipError('lrg_kitti_table_slots refused %d points' % n)
        return self.torch.empty(slots, dtype=self.torch.int64, device=self.dev), self.torch.empty(slots, dtype=self.torch.int32, device=self.dev), slots


def project_stack(scans, labels, images, poses, tr, p2, voxel_resolution, device='cuda:0', times=None):
    """Steps 2-5 (lrg_kitti_project).  scans: float32 [n_s, >= 3] per scan, labels: uint32 [n_s], images: uint8 [H, W, 3], poses: the 4x4
    matrices of read_poses.  Returns device tensors: xyz float64 [N, 3], rgb uint8 [N, 3], valid / keep bool [N], scan_of, obj, cls int32 [N]
    over all points in (scan, index) order."""
    D = _Dev(device)
    torch = D.torch
    S = len(scans)
    if S < 1 or not (len(labels) == len(images) == len(poses) == S):
        raise ValueError('project_stack: %d scans, %d label arrays, %d images, %d poses' % (S, len(labels), len(images), len(poses)))
    scans = [np.ascontiguousarray(s, dtype=np.float32) for s in scans]
    counts = [len(s) for s in scans]
    for s in range(S):
        if scans[s].ndim != 2 or scans[s].shape[1] < 3 or len(labels[s]) != counts[s]:
            raise ValueError('scan %d: points %s, %d labels' % (s, scans[s].shape, len(labels[s])))
        if images[s].ndim != 3 or images[s].shape[2] != 3 or images[s].dtype != np.uint8:
            raise ValueError('image %d: uint8 [H, W, 3] expected, got %s %s' % (s, images[s].dtype, images[s].shape))
    N = int(sum(counts))
    if N == 0:
        raise ValueError('project_stack: the scans hold no points')
    if N > _lib.LRG_KITTI_MAX_POINTS:
        raise ValueError('%d points in one stack (at most %d)' % (N, _lib.LRG_KITTI_MAX_POINTS))
    ld = scans[0].shape[1]
    if any(s.shape[1] != ld for s in scans):
        raise ValueError('scans of different widths')
    h_lab = np.concatenate([np.asarray(l, dtype=np.uint32) for l in labels]) if N else np.zeros(0, np.uint32)
    d_pts = torch.from_numpy(np.concatenate(scans) if N else np.zeros((0, ld), np.float32)).to(D.dev)
    d_lab = torch.from_numpy(h_lab.view(np.int32)).to(D.dev)
    d_scan = torch.from_numpy(np.repeat(np.arange(S, dtype=np.int32), counts)).to(D.dev)
    d_pose = torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(p, dtype=np.float64)[:3] for p in poses]).reshape(S, 12))).to(D.dev)
    d_tr = torch.from_numpy(np.ascontiguousarray(np.asarray(tr, dtype=np.float64).reshape(16))).to(D.dev)
    d_p2 = torch.from_numpy(np.ascontiguousarray(np.asarray(p2, dtype=np.float64)[:3].reshape(12))).to(D.dev)
    sizes = [im.size for im in images]
    d_img = torch.from_numpy(np.concatenate([np.ascontiguousarray(im).reshape(-1) for im in images])).to(D.dev)
    d_off = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)).to(D.dev)
    d_h = torch.tensor([im.shape[0] for im in images], dtype=torch.int32, device=D.dev)
    d_w = torch.tensor([im.shape[1] for im in images], dtype=torch.int32, device=D.dev)
    keys, vals, slots = D.table(N)
    xyz = torch.empty((N, 3), dtype=torch.float64, device=D.dev)
    rgb = torch.empty((N, 3), dtype=torch.uint8, device=D.dev)
    valid = torch.empty(N, dtype=torch.uint8, device=D.dev)
    keep = torch.empty(N, dtype=torch.uint8, device=D.dev)
    status = torch.zeros(1, dtype=torch.int32, device=D.dev)
    ev = _events(torch, times)
    _lib.check(D.lib.lrg_kitti_project(D.ptr(d_pts), ld, D.ptr(d_scan), D.ptr(d_lab), N, S, D.ptr(d_pose), D.ptr(d_tr), D.ptr(d_p2), D.ptr(d_img), D.ptr(d_off),
                                       D.ptr(d_h), D.ptr(d_w), float(voxel_resolution), D.ptr(keys), D.ptr(vals), slots, D.ptr(xyz), D.ptr(rgb), D.ptr(valid),
                                       D.ptr(keep), D.ptr(status), D.st), 'lrg_kitti_project')
    _record(ev, times, 'project_ms')
    _status(status, 'lrg_kitti_project')
    return dict(xyz=xyz, rgb=rgb, valid=valid.bool(), keep=keep.bool(), scan_of=d_scan, obj=(d_lab >> 16) & 0xFFFF, cls=d_lab & 0xFFFF, counts=counts)


def _kept_per_scan(pr, n_scans):
    """The kept points of every scan of a projected stack."""
    import torch
    return torch.bincount(pr['scan_of'][pr['keep']].long(), minlength=n_scans).tolist()


def kept_counts(scans, labels, images, poses, tr, p2, voxel_resolution, device='cuda:0', times=None):
    """Steps 2-5 alone, for a stack that never becomes a sample: the counts of its 'Processing' lines."""
    return _kept_per_scan(project_stack(scans, labels, images, poses, tr, p2, voxel_resolution, device=device, times=times), len(scans))


def _events(torch, times):
    if times is None:
        return None
    ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev[0].record()
    return ev


def _record(ev, times, name):
    if ev is not None:
        ev[1].record()
        ev[1].synchronize()
        times[name] = times.get(name, 0.0) + ev[0].elapsed_time(ev[1])


def first_in_voxel(xyz, resolution, device='cuda:0', times=None, name='first_in_voxel_ms'):
    """lrg_kitti_first_in_voxel: for float64 [n, 3] on the device, int32 [n] = the smallest index of every point's voxel."""
    D = _Dev(device)
    torch = D.torch
    xyz = xyz.contiguous()
    n = int(xyz.shape[0])
    keys, vals, slots = D.table(n)
    rep = torch.empty(n, dtype=torch.int32, device=D.dev)
    if n == 0:
        return rep
    status = torch.zeros(1, dtype=torch.int32, device=D.dev)
    ev = _events(torch, times)
    _lib.check(D.lib.lrg_kitti_first_in_voxel(D.ptr(xyz), n, float(resolution), D.ptr(keys), D.ptr(vals), slots, D.ptr(rep), D.ptr(status), D.st),
               'lrg_kitti_first_in_voxel')
    _record(ev, times, name)
    _status(status, 'lrg_kitti_first_in_voxel')
    return rep


def components(xyz, obj, cls, resolution, device='cuda:0', times=None):
    """lrg_kitti_components on equalised points: dict of int32 [n] root, size and first_src (both read at the roots) and bool emits."""
    D = _Dev(device)
    torch = D.torch
    xyz, obj, cls = xyz.contiguous(), obj.to(torch.int32).contiguous(), cls.to(torch.int32).contiguous()
    n = int(xyz.shape[0])
    keys, vals, slots = D.table(n)
    root, size, first_src = (torch.empty(n, dtype=torch.int32, device=D.dev) for _ in range(3))
    emits = torch.empty(n, dtype=torch.uint8, device=D.dev)
    if n == 0:
        return dict(root=root, size=size, first_src=first_src, emits=emits.bool())
    status = torch.zeros(1, dtype=torch.int32, device=D.dev)
    ev = _events(torch, times)
    _lib.check(D.lib.lrg_kitti_components(D.ptr(xyz), D.ptr(obj), D.ptr(cls), n, float(resolution), D.ptr(keys), D.ptr(vals), slots, D.ptr(root), D.ptr(size),
                                          D.ptr(first_src), D.ptr(emits), D.ptr(status), D.st), 'lrg_kitti_components')
    _record(ev, times, 'components_ms')
    _status(status, 'lrg_kitti_components')
    return dict(root=root, size=size, first_src=first_src, emits=emits.bool())


def original_ids(obj_column):
    """Step 8: the non-zero object ids in the order ``set(column) - set([0])`` iterates.  The set is built from the distinct values in the
    order they first appear: repeats do not change a set's table."""
    col = np.asarray(obj_column, dtype=np.float64)
    _, first = np.unique(col, return_index=True)
    distinct = col[np.sort(first)]
    return list(set(distinct) - set([0]))


def fuse_sample(scans, labels, images, poses, tr, p2, voxel_resolution=0.3, downsample_resolution=0.1, min_cluster=50, device='cuda:0',
                times=None):
    """Steps 2-10 for one sample; `poses` are read_poses' matrices (step 1).  Returns a dict: points float32 [rows, 8] (x y z r g b obj cls),
    kept_per_scan (the counts of the 'Processing' lines), n_equalized, n_original, n_labels (the numbers of the 'Creating' line) and
    `line`."""
    D = _Dev(device)
    torch = D.torch
    pr = project_stack(scans, labels, images, poses, tr, p2, voxel_resolution, device=device, times=times)
    kept_per_scan = _kept_per_scan(pr, len(scans))
    kept = torch.nonzero(pr['keep']).reshape(-1)                                                  # order-preserving compaction
    xyz, rgb, obj, cls = pr['xyz'][kept], pr['rgb'][kept], pr['obj'][kept], pr['cls'][kept]
    rep = first_in_voxel(xyz, downsample_resolution, device=device, times=times, name='downsample_ms')          # step 6
    first = torch.nonzero(rep == torch.arange(len(rep), device=D.dev, dtype=torch.int32)).reshape(-1)
    xyz, rgb, obj, cls = xyz[first], rgb[first], obj[first], cls[first]
    rep = first_in_voxel(xyz, voxel_resolution, device=device, times=times, name='equalize_ms')                 # step 7
    is_first = rep == torch.arange(len(rep), device=D.dev, dtype=torch.int32)
    equalized_idx = torch.nonzero(is_first).reshape(-1)
    unequalized_idx = (torch.cumsum(is_first.long(), 0) - 1)[rep.long()]
    e_xyz, e_obj, e_cls = xyz[equalized_idx], obj[equalized_idx], cls[equalized_idx]
    ids = original_ids(e_obj.cpu().numpy())                                                 # step 8
    table = np.zeros(1 << 16, dtype=np.int64)
    for k, o in enumerate(ids):
        table[int(o)] = k + 1
    new_obj = torch.from_numpy(table).to(D.dev)[e_obj.long()]
    comp = components(e_xyz, e_obj, e_cls, voxel_resolution, device=device, times=times)   # step 9
    n = len(e_obj)
    at_root = comp['root'].long() == torch.arange(n, device=D.dev)
    qualifies = at_root & (comp['first_src'] != np.iinfo(np.int32).max) & (comp['size'] > int(min_cluster))
    q_roots = torch.nonzero(qualifies).reshape(-1)
    order = torch.argsort(comp['first_src'][q_roots].long())                                # first sources are distinct: the order is total
    number = torch.zeros(n, dtype=torch.int64, device=D.dev)
    number[q_roots[order]] = torch.arange(len(q_roots), device=D.dev) + (len(ids) + 1)
    of_point = number[comp['root'].long()]
    new_obj = torch.where(of_point > 0, of_point, new_obj)
    label = new_obj[unequalized_idx]                                                        # step 10
    rows = torch.nonzero(label > 0).reshape(-1)
    out = torch.empty((len(rows), 8), dtype=torch.float64, device=D.dev)
    out[:, :3] = xyz[rows]
    out[:, 3:6] = torch.from_numpy(np.arange(256) / 255.0 - 0.5).to(D.dev)[rgb[rows].long()]      # rgb / 255.0 - 0.5 as NumPy rounds it
    out[:, 6] = label[rows].to(torch.float64)
    out[:, 7] = cls[rows].to(torch.float64)
    points = out.to(torch.float32).cpu().numpy()
    n_labels = int(torch.unique(new_obj).numel())
    return dict(points=points, kept_per_scan=kept_per_scan, n_downsampled=int(len(xyz)), n_equalized=n, n_original=len(ids), n_labels=n_labels,
                line='Creating data sample with %d->%d points %d->%d objects' % (len(points), n, len(ids), n_labels))


def _read_stack(scan_names, label_names, image_names, which, times=None):
    import time
    from . import io as lio
    t0 = time.perf_counter()
    scans = [np.fromfile(scan_names[i], dtype=np.float32).reshape((-1, 4)) for i in which]
    labels = [np.fromfile(label_names[i], dtype=np.uint32) for i in which]
    t1 = time.perf_counter()
    images = [lio.read_png(image_names[i]) for i in which]
    if times is not None:
        times['read_ms'] = times.get('read_ms', 0.0) + 1e3 * (t1 - t0)
        times['png_ms'] = times.get('png_ms', 0.0) + 1e3 * (time.perf_counter() - t1)
    return scans, labels, images


def stage_sequences(dataset, sequences, interval=20, skip=10, min_cluster=50, voxel_resolution=0.3, downsample_resolution=0.1, device='cuda:0',
                    log=print, times=None):
    """The sample loop of stage_semantic_kitti.py:41-202 over the listed sequences.  A sample is the stack of `interval` scans that ends at
    an offset with offset % interval == interval - 1; the next one starts skip * interval + 1 scans later; an unfinished stack at the end
    of a sequence is dropped (its 'Processing' lines are still printed).  Returns the rooms, float32 [rows, 8] each."""
    if interval < 1 or skip < 0:
        raise ValueError('interval must be at least 1 and skip at least 0')
    rooms = []
    for sequence in sequences:
        base = os.path.join(dataset, 'sequences', sequence)
        calib = read_calib(os.path.join(base, 'calib.txt'))
        poses = read_poses(os.path.join(base, 'poses.txt'), calib['Tr'])
        scan_names, label_names, image_names = list_sequence(dataset, sequence)
        if len(poses) < len(scan_names):
            raise ValueError('sequence %s: %d scans but %d poses' % (sequence, len(scan_names), len(poses)))
        offset = 0
        while offset < len(scan_names):
            which = list(range(offset, min(offset + interval, len(scan_names))))
            scans, labels, images = _read_stack(scan_names, label_names, image_names, which, times)
            args = (scans, labels, images, [poses[i] for i in which], calib['Tr'], calib['P2'], voxel_resolution)
            if len(which) == interval:
                res = fuse_sample(*args, downsample_resolution=downsample_resolution, min_cluster=min_cluster, device=device, times=times)
                counts = res['kept_per_scan']
            else:
                counts = kept_counts(*args, device=device, times=times)
            for i, c in zip(which, counts):
                log('Processing %d points from %s' % (c, scan_names[i][len(dataset):]))
            if len(which) == interval:
                log(res['line'])
                rooms.append(res['points'])
            offset += (skip + 1) * interval
    return rooms
