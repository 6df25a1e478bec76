"""Host twin of the KITTI staging: the ten rules restated with dicts and plain loops over Python floats, one point at a
time.  It shares no code with learn_region_grow_amd.kitti and keeps every intermediate the device kernels are tested against, together
with the counts that show which rules a sequence reaches."""
import numpy as np


def transform_poses(tr, raw_poses):
    """Rule 1: Tr^-1 pose Tr per scan."""
    tr_inv = np.linalg.inv(tr)
    return [np.matmul(tr_inv, np.matmul(p, tr)) for p in raw_poses]


def chain(row, x, y, z, w):
    return ((row[0] * x + row[1] * y) + row[2] * z) + row[3] * w


def voxel_of(p, res):
    return (round(p[0] / res), round(p[1] / res), round(p[2] / res))


def project_stack(scans, labels, images, poses, tr, p2, voxel_resolution):
    """Rules 2-5 for the scans of one stack.  scans: float32 [n, >=3] each, labels uint32 [n], images uint8 [H, W, 3], poses from
    transform_poses.  All points are numbered in (scan, index) order."""
    xyz, rgb, valid, keep, scan_of, obj, cls = [], [], [], [], [], [], []
    colour_map = {}                                   # voxel -> (colour, scan) of the first valid point
    cover = dict(invalid_from_map=0, invalid_refused_later=0, valid_black=0, moving=0)
    no_entry = []                                     # (point, voxel) of the invalid points that found no entry
    trr = [[float(v) for v in row] for row in np.asarray(tr)]
    p2r = [[float(v) for v in row] for row in np.asarray(p2)]
    for s in range(len(scans)):
        pose = [[float(v) for v in row] for row in np.asarray(poses[s])]
        image = images[s]
        H, W = image.shape[0], image.shape[1]
        first = len(xyz)
        vox = []
        for i in range(len(scans[s])):
            x, y, z = float(scans[s][i, 0]), float(scans[s][i, 1]), float(scans[s][i, 2])
            w = tuple(((pose[c][0] * x + pose[c][1] * y) + pose[c][2] * z) + pose[c][3] for c in range(3))
            cam = [chain(trr[c], x, y, z, 1.0) for c in range(4)]
            h = [chain(p2r[c], cam[0], cam[1], cam[2], cam[3]) for c in range(3)]
            ok, colour = False, (0, 0, 0)
            if h[2] > 0:
                u, v = float(round(h[0] / h[2])), float(round(h[1] / h[2]))
                ok = 0 <= u < W and 0 <= v < H
                if ok:
                    colour = tuple(int(c) for c in image[int(v), int(u), :3])
            xyz.append(w)
            rgb.append(colour)
            valid.append(ok)
            scan_of.append(s)
            vox.append(voxel_of(w, voxel_resolution))
            obj.append(int(labels[s][i]) >> 16)
            cls.append(int(labels[s][i]) & 0xFFFF)
        for i in range(first, len(xyz)):              # the scan's valid points enter the map first ...
            if valid[i] and vox[i - first] not in colour_map:
                colour_map[vox[i - first]] = (rgb[i], s)
        for i in range(first, len(xyz)):              # ... then its invalid points look themselves up
            if not valid[i]:
                if vox[i - first] in colour_map:
                    rgb[i] = colour_map[vox[i - first]][0]
                    cover['invalid_from_map'] += 1
                else:
                    no_entry.append(vox[i - first])
    cover['invalid_refused_later'] = sum(1 for k in no_entry if k in colour_map)
    for i in range(len(xyz)):
        black = rgb[i] == (0, 0, 0)
        if valid[i] and black:
            cover['valid_black'] += 1
        if cls[i] >= 250:
            cover['moving'] += 1
        keep.append(not black and cls[i] < 250)
    n = len(xyz)
    return dict(xyz=np.array(xyz, dtype=np.float64).reshape(n, 3), rgb=np.array(rgb, dtype=np.uint8).reshape(n, 3),
                valid=np.array(valid, dtype=bool), keep=np.array(keep, dtype=bool), scan_of=np.array(scan_of, dtype=np.int32),
                obj=np.array(obj, dtype=np.int64), cls=np.array(cls, dtype=np.int64), cover=cover,
                kept_per_scan=[int(np.sum(np.array(keep[a:b], dtype=bool))) for a, b in
                               zip(np.cumsum([0] + [len(s) for s in scans])[:-1], np.cumsum([len(s) for s in scans]))])


def first_in_voxel(xyz, res):
    """The smallest index of every point's voxel."""
    seen, rep = {}, []
    for i in range(len(xyz)):
        k = voxel_of((float(xyz[i, 0]), float(xyz[i, 1]), float(xyz[i, 2])), res)
        if k not in seen:
            seen[k] = i
        rep.append(seen[k])
    return np.array(rep, dtype=np.int64)


def components(xyz, obj, cls, res):
    """Rule 9 on equalised points: the edge list, then components in the order a graph built from that list meets its nodes."""
    n = len(xyz)
    vox = [voxel_of((float(xyz[i, 0]), float(xyz[i, 1]), float(xyz[i, 2])), res) for i in range(n)]
    where = {}
    for i in range(n):
        where[vox[i]] = i
    adj, emits, edges = {}, np.zeros(n, dtype=bool), []
    for i in range(n):
        if obj[i] > 0:
            continue
        k = vox[i]
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    if (dx, dy, dz) == (0, 0, 0):
                        continue
                    j = where.get((k[0] + dx, k[1] + dy, k[2] + dz))
                    if j is not None and cls[i] == cls[j]:
                        edges.append((i, j))
                        emits[i] = True
                        adj.setdefault(i, []).append(j)
                        adj.setdefault(j, []).append(i)
    clusters, seen = [], set()
    for start in adj:                                  # dicts keep insertion order: i, then j, edge by edge
        if start in seen:
            continue
        seen.add(start)
        members, stack = [start], [start]
        while stack:
            a = stack.pop()
            for b in adj[a]:
                if b not in seen:
                    seen.add(b)
                    members.append(b)
                    stack.append(b)
        clusters.append(members)
    root = np.arange(n)
    size_at, src_at = np.zeros(n, dtype=np.int64), np.full(n, np.iinfo(np.int32).max, dtype=np.int64)
    for members in clusters:
        r = min(members)
        root[members] = r
    for i in range(n):
        size_at[root[i]] += 1
        if emits[i]:
            src_at[root[i]] = min(src_at[root[i]], i)
    return dict(clusters=clusters, edges=edges, emits=emits, root=root, size=size_at, first_src=src_at)


def fuse_sample(scans, labels, images, poses, tr, p2, voxel_resolution, downsample_resolution, min_cluster):
    """Rules 2-10 for one sample.  Returns a dict: points float32 [rows, 8] and every intermediate."""
    pr = project_stack(scans, labels, images, poses, tr, p2, voxel_resolution)
    kept = np.nonzero(pr['keep'])[0]
    stacked = np.zeros((len(kept), 8))
    stacked[:, :3] = pr['xyz'][kept]
    stacked[:, 3:6] = pr['rgb'][kept].astype(np.float64) / 255.0 - 0.5
    stacked[:, 6] = pr['obj'][kept]
    stacked[:, 7] = pr['cls'][kept]
    rep_ds = first_in_voxel(stacked[:, :3], downsample_resolution)                 # rule 6
    ds = stacked[rep_ds == np.arange(len(stacked))]
    rep_eq = first_in_voxel(ds[:, :3], voxel_resolution)                           # rule 7
    equalized_idx = np.nonzero(rep_eq == np.arange(len(ds)))[0]
    rank = np.cumsum(rep_eq == np.arange(len(ds))) - 1
    unequalized_idx = rank[rep_eq]
    eq = ds[equalized_idx]
    obj, cls = eq[:, 6], eq[:, 7]
    new_obj = np.zeros(len(eq), dtype=np.int64)
    original = set(eq[:, 6]) - set([0])                                            # rule 8: Python's set order
    cluster_id = 1
    for o in original:
        new_obj[obj == o] = cluster_id
        cluster_id += 1
    comp = components(eq[:, :3], obj, cls, voxel_resolution)
    cover = dict(pr['cover'])
    cover.update(original_ids=len(original), labelled_overwritten=0, linked_through_labelled=0, small_component=0, component_at_threshold=0,
                 unlabelled_without_edge=int(np.sum(np.logical_and(obj == 0, ~comp['emits']))))
    # unlabelled groups: components of the edges whose two ends are unlabelled
    sub = np.arange(len(eq))

    def find(a):
        while sub[a] != a:
            sub[a] = sub[sub[a]]
            a = sub[a]
        return a
    for i, j in comp['edges']:
        if obj[j] == 0:
            a, b = find(i), find(j)
            if a != b:
                sub[max(a, b)] = min(a, b)
    for members in comp['clusters']:
        groups = set(find(i) for i in members if obj[i] == 0)
        if len(groups) > 1:
            cover['linked_through_labelled'] += 1
        if len(members) > min_cluster:
            cover['labelled_overwritten'] += int(np.sum(obj[members] > 0))
            new_obj[members] = cluster_id
            cluster_id += 1
            if len(members) == min_cluster + 1:
                cover['component_at_threshold'] += 1
        else:
            cover['small_component'] += 1
    ds = ds.copy()
    ds[:, 6] = new_obj[unequalized_idx]
    out = ds[ds[:, 6] > 0]
    return dict(points=out.astype(np.float32), project=pr, rep_ds=rep_ds, rep_eq=rep_eq, eq=eq, comp=comp, new_obj=new_obj,
                n_downsampled=len(ds), n_equalized=len(eq), n_original=len(original), n_labels=len(set(new_obj)), cover=cover,
                line='Creating data sample with %d->%d points %d->%d objects' % (len(out), len(eq), len(original), len(set(new_obj))))


def stage_sequence(scans, labels, images, names, raw_poses, tr, p2, interval, skip, min_cluster, voxel_resolution, downsample_resolution):
    """The sample loop of one sequence.  Returns (samples, lines, cover): samples are fuse_sample's dicts."""
    poses = transform_poses(tr, raw_poses)
    samples, lines, cover = [], [], {}
    offset = 0
    while offset + interval <= len(scans):
        sel = list(range(offset, offset + interval))
        res = fuse_sample([scans[i] for i in sel], [labels[i] for i in sel], [images[i] for i in sel], [poses[i] for i in sel], tr, p2,
                          voxel_resolution, downsample_resolution, min_cluster)
        for i, c in zip(sel, res['project']['kept_per_scan']):
            lines.append('Processing %d points from %s' % (c, names[i]))
        lines.append(res['line'])
        samples.append(res)
        for k, v in res['cover'].items():
            cover[k] = min(cover.get(k, v), v) if k == 'original_ids' else cover.get(k, 0) + v       # fewest ids of a sample; sums
        offset += (skip + 1) * interval
    rest = list(range(offset, len(scans)))
    cover['unfinished_scans'] = len(rest)
    if rest:                                          # an unfinished stack: its lines are printed, its points dropped
        pr = project_stack([scans[i] for i in rest], [labels[i] for i in rest], [images[i] for i in rest], [poses[i] for i in rest], tr, p2,
                           voxel_resolution)
        for i, c in zip(rest, pr['kept_per_scan']):
            lines.append('Processing %d points from %s' % (c, names[i]))
    return samples, lines, cover
