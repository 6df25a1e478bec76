"""Training tuples for LrgNet from labeled rooms -- the job of the reference's ``stage_data.py``.

Reference: stage_data.py:115-249.  Every ground-truth object of a room is grown from a random seed by an imperfect
teacher: the neighbours of the right object are accepted and the wrong inliers rejected, each decision flipped with a
probability that starts at 0.2-0.4 and decays by 0.01 per step (:139-140,:201-202), until the mask equals the object or
nothing is left to do.  Every step with a non-empty neighbourhood yields one tuple: the current points with their
"should be removed" flags and the neighbouring points with their "should be added" flags (:183-199), at most 1024 points
per side; afterwards x, y and the feature columns 6.. of both sides are centred on the medians of the inlier side
(:242-249).  File layout of ``data/staged_*.h5``: points / count / remove / neighbor_points / neighbor_count / add / steps /
complete (:251-258), read back by train_region_grow.py:71-125.

``stage_room`` is the reference's loop on the host with the reference's stream; ``stage_rooms_gpu`` runs the same loop for all rooms of a
file on the device under the counter stream (csrc/lrg_stage.hip).  ``stage_data.py`` at the repository root drives both.
"""
import numpy as np

from . import h5lite


def stage_room(points, obj_id, rs, resolution=0.1, cluster_threshold=10, max_points=1024, max_steps=500, log=None):
    """points [N,F] (13-feature rows as the loop sees them), obj_id [N]; rs: numpy RandomState.
    Returns dict of lists: points, remove, neighbor_points, add (one entry per tuple), steps (per object), complete (IoU per tuple)."""
    points = np.asarray(points, dtype=np.float32)
    obj_id = np.asarray(obj_id)
    N = len(points)
    point_voxels = np.round(points[:, :3] / resolution).astype(int)
    visited = np.zeros(N, dtype=bool)
    out = dict(points=[], remove=[], neighbor_points=[], add=[], steps=[], complete=[])
    for seed_id in rs.choice(range(N), N, replace=False):                                  # :117
        if visited[seed_id]:
            continue
        target_id = obj_id[seed_id]
        gt_mask = obj_id == target_id
        currentMask = np.zeros(N, dtype=bool)
        currentMask[seed_id] = True
        minDims = point_voxels[seed_id].copy()
        maxDims = point_voxels[seed_id].copy()
        steps, stuck = 0, False
        add_mistake_prob = rs.randint(2, 5) * 0.1                                          # :139
        remove_mistake_prob = rs.randint(2, 5) * 0.1                                       # :140
        iou = 0.0
        while True:
            currentPoints = points[currentMask]
            mask = np.logical_and(np.all(point_voxels >= minDims - 1, axis=1), np.all(point_voxels <= maxDims + 1, axis=1))   # :153-158
            mask &= ~currentMask
            mask &= ~visited
            expandPoints = points[mask]
            expandClass = obj_id[mask] == target_id
            mask_idx = np.nonzero(mask)[0]
            if stuck:                                                                       # :164-170
                expandID = mask_idx[expandClass]
            else:
                mistake = rs.random_sample(len(mask_idx)) < add_mistake_prob
                expandID = mask_idx[np.logical_xor(expandClass, mistake)]
            rejectClass = obj_id[currentMask] != target_id                                  # :173-181
            cur_idx = np.nonzero(currentMask)[0]
            if stuck:
                rejectID = cur_idx[rejectClass]
            else:
                mistake = rs.random_sample(len(cur_idx)) < remove_mistake_prob
                rejectID = cur_idx[np.logical_xor(rejectClass, mistake)]
            if len(expandPoints) > 0:                                                       # :183-202
                if len(currentPoints) <= max_points:
                    out['points'].append(currentPoints.copy())
                    out['remove'].append(rejectClass.astype(np.int32))
                else:
                    subset = rs.choice(len(currentPoints), max_points, replace=False)
                    out['points'].append(currentPoints[subset])
                    rejectClass = rejectClass[subset]
                    out['remove'].append(rejectClass.astype(np.int32))
                if len(expandPoints) <= max_points:
                    out['neighbor_points'].append(expandPoints.copy())
                    out['add'].append(expandClass.astype(np.int32))
                else:
                    subset = rs.choice(len(expandPoints), max_points, replace=False)
                    out['neighbor_points'].append(expandPoints[subset])
                    expandClass = expandClass[subset]
                    out['add'].append(expandClass.astype(np.int32))
                iou = 1.0 * np.sum(currentMask & gt_mask) / np.sum(currentMask | gt_mask)
                out['complete'].append(iou)
                steps += 1
                add_mistake_prob = max(add_mistake_prob - 0.01, 0.0)
                remove_mistake_prob = max(remove_mistake_prob - 0.01, 0.0)
            if np.all(currentMask == gt_mask):                                              # :204-210 completed
                visited[currentMask] = True
                out['steps'].append(steps)
                break
            if steps < max_steps and (np.any(expandClass) or np.any(rejectClass)):          # :212-227 keep growing
                currentMask[expandID] = True
                if len(rejectID) < len(cur_idx):
                    currentMask[rejectID] = False
                nextMin = point_voxels[currentMask].min(axis=0)
                nextMax = point_voxels[currentMask].max(axis=0)
                if not np.any(nextMin < minDims) and not np.any(nextMax > maxDims):
                    stuck = True
                minDims, maxDims = nextMin, nextMax
            else:                                                                           # :228-236 early termination
                if np.sum(currentMask) > cluster_threshold:
                    visited[currentMask] = True
                    out['steps'].append(steps)
                break
        if log is not None:
            log('target %d: %d steps %d/%d' % (target_id, steps, int(currentMask.sum()), int(gt_mask.sum())))
    return out


def center_tuples(staged):
    """stage_data.py:242-249, in place: x, y and the columns 6.. of both sides minus the inlier side's medians."""
    for i in range(len(staged['points'])):
        p = staged['points'][i]
        center = np.median(p[:, :2], axis=0)
        feature_center = np.median(p[:, 6:], axis=0)
        p[:, :2] -= center
        p[:, 6:] -= feature_center
        q = staged['neighbor_points'][i]
        if len(q) > 0:
            q[:, :2] -= center
            q[:, 6:] -= feature_center
    return staged


def merge(parts):
    out = dict(points=[], remove=[], neighbor_points=[], add=[], steps=[], complete=[])
    for p in parts:
        for k in out:
            out[k].extend(p[k])
    return out


def save_staged(filename, staged):
    """The datasets of data/staged_*.h5 (stage_data.py:251-258)."""
    F = staged['points'][0].shape[1] if staged['points'] else 13
    h5lite.write_file(filename, {
        'points': np.vstack(staged['points']).astype(np.float32) if staged['points'] else np.zeros((0, F), np.float32),
        'count': np.array([len(p) for p in staged['points']], dtype=np.int32),
        'neighbor_points': np.vstack(staged['neighbor_points']).astype(np.float32) if staged['neighbor_points'] else np.zeros((0, F), np.float32),
        'neighbor_count': np.array([len(p) for p in staged['neighbor_points']], dtype=np.int32),
        'add': np.concatenate(staged['add']).astype(np.int32) if staged['add'] else np.zeros(0, np.int32),
        'remove': np.concatenate(staged['remove']).astype(np.int32) if staged['remove'] else np.zeros(0, np.int32),
        'steps': np.array(staged['steps'], dtype=np.int32),
        'complete': np.array(staged['complete'], dtype=np.float32)})


def load_staged(filename, feature_size=13):
    """train_region_grow.py:71-125: the per-tuple arrays, tuples with an empty neighbourhood dropped (:128-133)."""
    f = h5lite.File(filename)
    count, ncount = f['count'].read(), f['neighbor_count'].read()
    pts, npts = f['points'].read(), f['neighbor_points'].read()
    rem, add = f['remove'].read(), f['add'].read()
    P = np.split(pts[:, :feature_size], np.cumsum(count)[:-1]) if len(count) else []
    R = np.split(rem, np.cumsum(count)[:-1]) if len(count) else []
    Q = np.split(npts[:, :feature_size], np.cumsum(ncount)[:-1]) if len(ncount) else []
    A = np.split(add, np.cumsum(ncount)[:-1]) if len(ncount) else []
    keep = [i for i in range(len(ncount)) if ncount[i] > 0]
    return dict(points=[P[i] for i in keep], remove=[R[i] for i in keep], neighbor_points=[Q[i] for i in keep], add=[A[i] for i in keep])


def assemble_batch(data, order, rs, batch_size=100, n_inlier=512, n_neighbor=512):
    """train_region_grow.py:156-175: every tuple of the batch padded / subsampled to the network's point counts with the legacy
    generator in the reference's call order (inlier choice, then neighbour choice, per tuple).
    -> inlier [B,Ni,F], neighbor [B,Nn,F] float32, input_add [B,Nn], input_remove [B,Ni] int32."""
    F = data['points'][0].shape[1]
    xi = np.zeros((batch_size, n_inlier, F), dtype=np.float32)
    xn = np.zeros((batch_size, n_neighbor, F), dtype=np.float32)
    ia = np.zeros((batch_size, n_neighbor), dtype=np.int32)
    ir = np.zeros((batch_size, n_inlier), dtype=np.int32)
    for i in range(batch_size):
        k = order[i]
        N = len(data['points'][k])
        subset = rs.choice(N, n_inlier, replace=False) if N >= n_inlier else list(range(N)) + list(rs.choice(N, n_inlier - N, replace=True))
        xi[i] = data['points'][k][subset]
        ir[i] = np.asarray(data['remove'][k])[subset]
        N = len(data['neighbor_points'][k])
        subset = rs.choice(N, n_neighbor, replace=False) if N >= n_neighbor else list(range(N)) + list(rs.choice(N, n_neighbor - N, replace=True))
        xn[i] = data['neighbor_points'][k][subset]
        ia[i] = np.asarray(data['add'][k])[subset]
    return xi, xn, ia, ir


def seed_transform(points, seed):
    """stage_data.py:50-56 on a copy of the raw points, before equalisation and the normals.  The reference is Python 2, so SEED/2%2 and
    SEED/4==1 are integer expressions: x and y swapped for seeds 1, 3, 5, 7, then x negated for 2, 3, 6, 7, then y negated for 4 .. 7."""
    p = np.array(points, copy=True)
    if seed is None:
        return p
    if seed % 2 == 1:
        p[:, [0, 1]] = p[:, [1, 0]]
    if seed // 2 % 2 == 1:
        p[:, 0] = -p[:, 0]
    if seed // 4 == 1:
        p[:, 1] = -p[:, 1]
    return p


STAGE_ARENA_PER_POINT = 192         # first arena of a room, list entries per point (Area-5-shaped rooms of 2-6 k points emit 60-150); doubled on OVERFLOW
STAGE_ARENA_LAUNCH = 1 << 30        # list entries of one teacher launch (the tuple table holds 32-bit offsets)


def stage_rooms_gpu(rooms, seed=0, resolution=0.1, max_points=1024, device='cuda:0', cluster_threshold=10, max_steps=500, max_iters=None,
                    arena_entries=None, info=None, download=True):
    """The device teacher (csrc/lrg_stage.hip) under the counter stream keyed by (seed, room_id): lrg_stage_teacher over all rooms in one
    launch, then lrg_stage_tuples over all their tuples.  rooms: dicts with points [n,F] float32, obj_id [n] and optionally room_id (default:
    the position in the list).  Returns the dict `merge` returns, rows already centred (stage_data.py:233-240); `save_staged` takes it as it is.
    arena_entries: first arena of every room in list entries (default STAGE_ARENA_PER_POINT per point); a room whose tuples overrun its arena
    is run again with twice as much -- the draws are pure functions, the repeat gives the same tuples.
    info (a dict) collects 'launches', 'overflowed' (room positions), 'bytes_downloaded', 'teacher_ms' / 'tuples_ms' (device time by events),
    'tuples' and 'objects' (per room the int32 rows steps, seed, points, IoU bits of its stored objects).
    download=False leaves the rows where lrg_stage_tuples wrote them: the per-tuple lists stay empty and the result has 'device' = dict of the
    flat device buffers points [rows,F] / remove [rows] / neighbor_points [rows,F] / add [rows] and the host tables row_in / row_nb [T+1] int64
    (tuple t's rows are row_in[t] .. row_in[t+1]); train_data.TupleStore.from_device takes it.  steps, complete and info as before;
    bytes_downloaded then counts status, headers and objects only."""
    import ctypes
    import torch
    from . import _lib
    lib = _lib.load()
    if not torch.cuda.is_available():
        raise _lib.LrgHipError('stage_rooms_gpu needs a GPU (the legacy stream stages on the host: stage_room)')
    if not 1 <= max_points <= _lib.LRG_STAGE_MAX_POINTS:
        raise ValueError('max_points must be 1 .. %d' % _lib.LRG_STAGE_MAX_POINTS)
    if info is None:
        info = {}
    info.update(launches=0, overflowed=[], bytes_downloaded=0, teacher_ms=0.0, tuples_ms=0.0, tuples=0, objects=[])
    out = dict(points=[], remove=[], neighbor_points=[], add=[], steps=[], complete=[])

    def left_on_device(d_p, d_r, d_q, d_a, row_in, row_nb):
        return dict(points=d_p, remove=d_r, neighbor_points=d_q, add=d_a, row_in=np.asarray(row_in, dtype=np.int64), row_nb=np.asarray(row_nb, dtype=np.int64))

    def nothing_on_device(F):
        d = torch.device(device)
        return left_on_device(torch.empty((0, F), dtype=torch.float32, device=d), torch.empty(0, dtype=torch.int32, device=d),
                              torch.empty((0, F), dtype=torch.float32, device=d), torch.empty(0, dtype=torch.int32, device=d), [0], [0])
    if not rooms:
        if not download:
            out['device'] = nothing_on_device(13)
        return out
    if max_iters is None:
        max_iters = 2 * max_steps + 64
    dev = torch.device(device)
    torch.cuda.set_device(dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def ptr(t):
        return ctypes.c_void_p(t.data_ptr())
    ns = [int(len(r['points'])) for r in rooms]
    F = int(np.asarray(rooms[0]['points']).shape[1])
    if min(ns) < 1 or max(ns) >= 1 << 30:
        raise ValueError('rooms of 1 .. 2^30 - 1 points')
    offs = np.concatenate([[0], np.cumsum([(n + 15) // 16 * 16 for n in ns])]).astype(np.int64)
    tot = int(offs[-1])
    pts = np.zeros((tot, F), dtype=np.float32)
    obj = np.zeros(tot, dtype=np.int32)
    for r, room in enumerate(rooms):
        p = np.asarray(room['points'], dtype=np.float32)
        if p.shape != (ns[r], F):
            raise ValueError('room %d: points of shape %s, expected %s' % (r, p.shape, (ns[r], F)))
        pts[offs[r]:offs[r] + ns[r]] = p
        obj[offs[r]:offs[r] + ns[r]] = np.asarray(room['obj_id']).astype(np.int32)
    d_points, d_obj = torch.from_numpy(pts).to(dev), torch.from_numpy(obj).to(dev)
    d_vox = torch.empty((tot, 3), dtype=torch.int32, device=dev)
    _lib.check(lib.lrg_voxelize(ptr(d_points), tot, F, ctypes.c_float(resolution), ptr(d_vox), st), 'lrg_voxelize')
    d_visited = torch.zeros(tot, dtype=torch.uint8, device=dev)
    d_cur = torch.zeros(tot, dtype=torch.uint8, device=dev)
    d_lists = torch.empty(2 * tot, dtype=torch.int32, device=dev)
    d_objects = torch.zeros((tot, 4), dtype=torch.int32, device=dev)
    d_status = torch.zeros((len(rooms), 4), dtype=torch.int32, device=dev)
    h_rooms = (_lib.LrgRoom * len(rooms))()
    room_ids = []
    for r, room in enumerate(rooms):
        R, o = h_rooms[r], int(offs[r])
        R.points = d_points.data_ptr() + o * F * 4
        R.voxels = d_vox.data_ptr() + o * 12
        R.obj_id = d_obj.data_ptr() + o * 4
        R.visited = d_visited.data_ptr() + o
        R.n = ns[r]
        R.room_id = int(room.get('room_id', r))
        room_ids.append(int(R.room_id))
    d_rooms = torch.from_numpy(np.frombuffer(bytes(h_rooms), dtype=np.uint8).copy()).to(dev)
    d_ws_off = torch.from_numpy(offs[:-1].copy()).to(dev)
    caps = [int(arena_entries) if arena_entries else max(1 << 16, STAGE_ARENA_PER_POINT * n) for n in ns]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    # ---- the teacher: every room until its arena holds all its tuples ----
    done = {}                     # room -> (arena tensor, its offset there, headers [T,8] uint32 on the host)
    todo = list(range(len(rooms)))
    while todo:
        group, words = [], 0
        while todo and (not group or words + caps[todo[0]] <= STAGE_ARENA_LAUNCH):
            if caps[todo[0]] > STAGE_ARENA_LAUNCH:
                raise _lib.LrgHipError('room %d (room_id %d) needs an arena above %d entries' % (todo[0], room_ids[todo[0]], STAGE_ARENA_LAUNCH))
            words += caps[todo[0]]
            group.append(todo.pop(0))
        a_off = np.zeros(len(rooms), dtype=np.int64)
        a_cap = np.zeros(len(rooms), dtype=np.int32)
        a_off[group] = np.concatenate([[0], np.cumsum([caps[r] for r in group])[:-1]])
        a_cap[group] = [caps[r] for r in group]
        d_arena = torch.empty(words, dtype=torch.int32, device=dev)
        d_list = torch.tensor(group, dtype=torch.int32, device=dev)
        d_aoff, d_acap = torch.from_numpy(a_off).to(dev), torch.from_numpy(a_cap).to(dev)
        ev[0].record()
        _lib.check(lib.lrg_stage_teacher(ptr(d_rooms), ptr(d_list), len(group), ptr(d_ws_off), ptr(d_cur), ptr(d_lists), ptr(d_arena), ptr(d_aoff),
                                         ptr(d_acap), ptr(d_objects), ptr(d_status), ctypes.c_uint32(int(seed) & 0xFFFFFFFF), max_points,
                                         cluster_threshold, max_steps, max_iters, st), 'lrg_stage_teacher')
        ev[1].record()
        status = d_status.cpu().numpy()
        info['launches'] += 1
        info['teacher_ms'] += ev[0].elapsed_time(ev[1])
        info['bytes_downloaded'] += status.nbytes
        again, idx = [], []
        for r in group:
            if status[r, 0] == _lib.LRG_STAGE_ITER_CAP:
                raise _lib.LrgHipError('room %d (room_id %d): an object\'s loop reached max_iters = %d passes (LRG_STAGE_ITER_CAP)' % (r, room_ids[r], max_iters))
            if status[r, 0] == _lib.LRG_STAGE_OVERFLOW:
                caps[r] *= 2
                again.append(r)
                info['overflowed'].append(r)
                continue
            if status[r, 0] != _lib.LRG_STAGE_OK:
                raise _lib.LrgHipError('room %d: status %d' % (r, status[r, 0]))
            T = int(status[r, 1])
            idx.append((a_off[r] + a_cap[r] - 8 * (np.arange(T, dtype=np.int64) + 1))[:, None] + np.arange(8, dtype=np.int64)[None, :])
        hdr = np.zeros((0, 8), dtype=np.int32)
        if idx and sum(len(i) for i in idx):
            hdr = d_arena[torch.from_numpy(np.concatenate(idx).reshape(-1)).to(dev)].cpu().numpy().reshape(-1, 8)
            info['bytes_downloaded'] += hdr.nbytes
        pos = 0
        for r in group:
            if r in again:
                continue
            T = int(status[r, 1])
            done[r] = (d_arena, int(a_off[r]), hdr[pos:pos + T], int(status[r, 3]))
            pos += T
        todo = again + todo
    # ---- the stored objects ----
    oidx = np.concatenate([offs[r] + np.arange(done[r][3], dtype=np.int64) for r in range(len(rooms))])
    objects = d_objects[torch.from_numpy(oidx).to(dev)].cpu().numpy() if len(oidx) else np.zeros((0, 4), dtype=np.int32)
    info['bytes_downloaded'] += objects.nbytes
    pos = 0
    for r in range(len(rooms)):
        info['objects'].append(objects[pos:pos + done[r][3]])
        pos += done[r][3]
    out['steps'] = [int(s) for s in objects[:, 0]]
    # ---- the rows: one workgroup per tuple, offsets from a prefix sum of the headers ----
    hdr_all = np.concatenate([done[r][2] for r in range(len(rooms))]) if done else np.zeros((0, 8), dtype=np.int32)
    T = len(hdr_all)
    info['tuples'] = T
    if T == 0:
        if not download:
            out['device'] = nothing_on_device(F)
        return out
    cnt_in, cnt_nb = hdr_all[:, 0].astype(np.int64), hdr_all[:, 1].astype(np.int64)
    row_in = np.concatenate([[0], np.cumsum(cnt_in)])
    row_nb = np.concatenate([[0], np.cumsum(cnt_nb)])
    if row_in[-1] >= 1 << 31 or row_nb[-1] >= 1 << 31:
        raise _lib.LrgHipError('more than 2^31 staged rows in one call: stage fewer rooms at a time')
    d_p = torch.empty((int(row_in[-1]), F), dtype=torch.float32, device=dev)
    d_r = torch.empty(int(row_in[-1]), dtype=torch.int32, device=dev)
    d_q = torch.empty((int(row_nb[-1]), F), dtype=torch.float32, device=dev)
    d_a = torch.empty(int(row_nb[-1]), dtype=torch.int32, device=dev)
    first = np.concatenate([[0], np.cumsum([len(done[r][2]) for r in range(len(rooms))])])
    by_arena = {}
    for r in range(len(rooms)):
        by_arena.setdefault(id(done[r][0]), []).append(r)
    for rs_ in by_arena.values():
        rows = []
        for r in rs_:
            h, t0 = done[r][2], int(first[r])
            if not len(h):
                continue
            tab = np.zeros((len(h), 8), dtype=np.int32)
            tab[:, 0] = r
            tab[:, 1], tab[:, 2] = h[:, 0], h[:, 1]
            tab[:, 3], tab[:, 4] = done[r][1] + h[:, 2], done[r][1] + h[:, 3]
            tab[:, 5], tab[:, 6] = row_in[t0:t0 + len(h)], row_nb[t0:t0 + len(h)]
            rows.append(tab)
        if not rows:
            continue
        d_tab = torch.from_numpy(np.concatenate(rows)).to(dev)
        ev[0].record()
        _lib.check(lib.lrg_stage_tuples(ptr(d_rooms), ptr(done[rs_[0]][0]), ptr(d_tab), int(d_tab.shape[0]), F, ptr(d_p), ptr(d_r), ptr(d_q), ptr(d_a), st),
                   'lrg_stage_tuples')
        ev[1].record()
        ev[1].synchronize()
        info['tuples_ms'] += ev[0].elapsed_time(ev[1])
    out['complete'] = list(hdr_all[:, 4].copy().view(np.float32))
    if not download:
        out['device'] = left_on_device(d_p, d_r, d_q, d_a, row_in, row_nb)
        return out
    h_p, h_r, h_q, h_a = d_p.cpu().numpy(), d_r.cpu().numpy(), d_q.cpu().numpy(), d_a.cpu().numpy()
    info['bytes_downloaded'] += h_p.nbytes + h_r.nbytes + h_q.nbytes + h_a.nbytes
    out['points'] = np.split(h_p, row_in[1:-1])
    out['remove'] = np.split(h_r, row_in[1:-1])
    out['neighbor_points'] = np.split(h_q, row_nb[1:-1])
    out['add'] = np.split(h_a, row_nb[1:-1])
    return out
