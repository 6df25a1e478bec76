"""h5_to_ply.py and examine_h5.py of the reference's "Data Visualization" section: the rooms of an HDF5 room file as PLY clouds in scan
colours (--rgb), ground-truth instances ordered by size (--seg) or class colours (--cls), and the legend of one room (--target N).

All rooms of the file go through one batched device pass: the equalisation of h5_to_ply.py:72-84 is lrg_preprocess_batch's
(equalized_idx / unequalized_idx as it stands), the colours are torch operations on the device, and the vertex lines are encoded by
lrg_text_encode (io.save_rooms_ply_device).  What stays on the host is small: the ranking of a room's objects by size is
``unique_id[numpy.argsort(count)][::-1]`` (:97) on the device histogram's counts -- NumPy's order among equal counts is not imitated on
the device -- and the legend lines of --target.

The reference keeps its class names and class colours as tables in its program text; here they come from a file, --class-table, with
lines ``id name r g b``.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

from . import h5lite

EXCLUDED_FROM_LEGEND = ('ceiling', 'none', 'unlabeled')      # h5_to_ply.py:100


def examine(filename, out=sys.stdout):
    """examine_h5.py: every dataset as h5py prints it, and its minimum, mean and maximum."""
    f = h5lite.File(filename)
    for k in f.keys():
        d = f[k]
        out.write('<HDF5 dataset "%s": shape %s, type "%s">\n' % (k, tuple(int(s) for s in d.shape), np.dtype(d.dtype).str))
        l = d.read()
        out.write('min %.2f mean %.2f max %.2f\n' % (l.min(), l.mean(), l.max()))


def read_class_table(filename):
    """Lines ``id name r g b`` (blank lines and lines starting with # skipped): names {id: name} and colours [max id + 1, 3] int32
    (rows nobody names stay -1)."""
    names, rows = {}, {}
    with open(filename) as f:
        for no, ln in enumerate(f, 1):
            t = ln.split()
            if not t or t[0].startswith('#'):
                continue
            try:
                if len(t) != 5:
                    raise ValueError
                i, rgb = int(t[0]), [int(v) for v in t[2:5]]
                if i < 0 or i in names:
                    raise ValueError
            except ValueError:
                raise ValueError('%s:%d: "id name r g b" expected, one line per class id' % (filename, no))
            names[i], rows[i] = t[1], rgb
    if not names:
        raise ValueError('%s names no class' % filename)
    colours = np.full((max(names) + 1, 3), -1, dtype=np.int32)
    for i, rgb in rows.items():
        colours[i] = rgb
    return names, colours


def rank_objects(count_per_id):
    """h5_to_ply.py:90-97 on the histogram of a room's equalised object ids: (shift, ranked) -- shift = 1 if the smallest id is 0 (the
    reference then adds 1 to every id), ranked = the shifted ids, largest object first, in NumPy's own order among equal counts."""
    count_per_id = np.asarray(count_per_id)
    unique_id = np.nonzero(count_per_id)[0]
    count = count_per_id[unique_id]
    shift = 1 if unique_id[0] == 0 else 0
    unique_id = unique_id + shift
    return shift, unique_id[np.argsort(count)][::-1]


def object_colours(ranked, max_id):
    """Colour per shifted object id [max_id + 1, 3]: obj_color[k + 1] for the k-th largest (:93,:102,:108), row 0 grey (:107)."""
    obj_color = np.random.RandomState(0).randint(0, 255, (max_id + 1, 3))
    obj_color[0, :] = [100, 100, 100]
    table = np.zeros((max_id + 1, 3), dtype=np.int32)
    table[ranked] = obj_color[1:len(ranked) + 1]
    return table


class RoomFile:
    """The rooms of an HDF5 room file on the device, equalised in one lrg_preprocess_batch call."""

    def __init__(self, filename, resolution=0.1, device='cuda:0', rooms=None):
        import torch
        from . import _lib
        from .lrgnet import _ptr, _stream_ptr
        f = h5lite.File(filename)
        rows, counts = f['points'].read(), f['count_room'].read().astype(np.int64)
        if rows.ndim != 2 or rows.shape[1] < 8:
            raise ValueError("%s: 'points' [n, >= 8] (x y z r g b ... object class) expected, got %s" % (filename, rows.shape))
        if counts.sum() != len(rows) or (counts < 0).any():
            raise ValueError("%s: 'count_room' does not add up to the rows of 'points'" % filename)
        bounds = np.concatenate([[0], np.cumsum(counts)])
        ids = list(range(len(counts))) if rooms is None else list(rooms)
        for r in ids:
            if not 0 <= r < len(counts):
                raise ValueError('%s has %d rooms: no room %d' % (filename, len(counts), r))
            if counts[r] == 0:
                raise ValueError('room %d of %s is empty' % (r, filename))
        self.room_ids, self.dev = ids, torch.device(device)
        if not torch.cuda.is_available():
            raise _lib.LrgHipError('h5_to_ply needs a GPU: there is no CPU fallback')
        if rooms is not None:
            rows = np.concatenate([rows[bounds[r]:bounds[r + 1]] for r in ids])
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        R, M, C = len(ids), len(rows), rows.shape[1]
        self.sizes = [int(counts[r]) for r in ids]
        self.raw_start = np.zeros(R + 1, dtype=np.int32)
        np.cumsum(self.sizes, out=self.raw_start[1:])
        if R == 0:
            return
        lib, dev = _lib.load(), self.dev
        rs_p = self.raw_start.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        nbytes = lib.lrg_preprocess_batch_workspace_bytes(rs_p, R)
        if nbytes == 0:
            raise _lib.LrgHipError('lrg_preprocess_batch: %d rooms with %d raw points do not fit one call' % (R, M))
        with torch.cuda.device(dev):
            self.rows = torch.from_numpy(rows).to(dev)
            obj, cls = self.rows[:, -2].to(torch.int32), self.rows[:, -1].to(torch.int32)      # astype(int) of :22-23: truncation
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            eq, self.uneq = torch.empty(M, dtype=torch.int32, device=dev), torch.empty(M, dtype=torch.int32, device=dev)
            cov = torch.empty((M, 9), dtype=torch.float64, device=dev)          # (eig_mode 0 is the pass that stops soonest; its covariances are not used)
            eqs = torch.empty(R + 1, dtype=torch.int32, device=dev)
            st = _stream_ptr(dev)
            _lib.check(lib.lrg_preprocess_batch(_ptr(self.rows), C, None, None, rs_p, R, ctypes.c_float(resolution), 6, 0, _ptr(ws), ws.numel(),
                                                None, None, None, None, _ptr(eq), _ptr(self.uneq), _ptr(cov), _ptr(eqs), None, st),
                       'lrg_preprocess_batch')
            status = (ctypes.c_int32 * R)()
            _lib.check(lib.lrg_preprocess_batch_status(_ptr(ws), rs_p, R, status, st), 'lrg_preprocess_batch_status')
            bad = [ids[k] for k in range(R) if status[k]]
            if bad:
                raise _lib.LrgHipError('room %s: a point lies outside the +-2^20 voxel window at resolution %g' % (', '.join(str(b) for b in bad), resolution))
            self.eq_start = eqs.cpu().numpy().astype(np.int64)
            N = int(self.eq_start[-1])
            room_of_raw = torch.repeat_interleave(torch.arange(R, device=dev), torch.as_tensor(self.sizes, device=dev))
            # the equalised row, among all rooms', of every raw point (:81: unequalized_idx is room-relative)
            self.raw_to_eq = torch.as_tensor(self.eq_start[:-1], device=dev)[room_of_raw] + self.uneq.to(torch.int64)
            self.room_of_eq = torch.repeat_interleave(torch.arange(R, device=dev), torch.as_tensor(np.diff(self.eq_start), device=dev))
            # :83-84 obj_id[equalized_idx], cls_id[equalized_idx] (equalized_idx is room-relative; the ids are gathered here: eig_mode 0 writes none)
            first = torch.as_tensor(self.raw_start[:-1].astype(np.int64), device=dev)[self.room_of_eq] + eq[:N].to(torch.int64)
            self.obj_eq, self.cls_eq = obj[first], cls[first]

    def xyz(self):
        return self.rows[:, :3]

    def room_slices(self, t):
        return [t[int(a):int(b)] for a, b in zip(self.raw_start[:-1], self.raw_start[1:])]

    def scan_colours(self):
        """(c + 0.5) * 255 in float32 (:87: the assignment into the float32 array), truncated as %d truncates."""
        import torch
        return ((self.rows[:, 3:6] + 0.5) * 255).to(torch.int32)

    def ranked_objects(self, k):
        """Room k (of this object's rooms): (shift, ranked ids, largest first) from the device histogram of its equalised object ids."""
        import torch
        ids = self.obj_eq[int(self.eq_start[k]):int(self.eq_start[k + 1])]
        if int(ids.min().item()) < 0:
            raise ValueError('room %d: a negative object id' % self.room_ids[k])
        return rank_objects(torch.bincount(ids.to(torch.int64)).cpu().numpy())

    def instance_colours(self):
        """:90-108: the colour of every raw point's voxel's first point's object, objects coloured by their rank in size."""
        import torch
        R = len(self.room_ids)
        tables, base, shifts = [], np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int64)
        for k in range(R):
            shift, ranked = self.ranked_objects(k)
            t = object_colours(ranked, int(ranked.max()))
            base[k], shifts[k] = sum(len(x) for x in tables), shift
            tables.append(t)
        dev = self.dev
        table = torch.from_numpy(np.concatenate(tables)).to(dev)
        row = torch.as_tensor(base + shifts, device=dev)[self.room_of_eq] + self.obj_eq.to(torch.int64)
        return table[row][self.raw_to_eq]

    def class_colours(self, colours):
        """:111: the table's colour of every raw point's voxel's first point's class."""
        import torch
        cls = self.cls_eq.to(torch.int64)
        table = torch.from_numpy(np.ascontiguousarray(colours, dtype=np.int32)).to(self.dev)
        lo, hi = int(cls.min().item()), int(cls.max().item())
        if lo < 0 or hi >= len(table) or int(table[cls].min().item()) < 0:
            raise ValueError('the file has a class id the class table does not name (ids %d .. %d)' % (lo, hi))
        return table[cls][self.raw_to_eq]

    def legend(self, k, names):
        """--target: one line per object of room k, largest first, without ceiling / none / unlabeled (:98-101)."""
        a, b = int(self.eq_start[k]), int(self.eq_start[k + 1])
        shift, ranked = self.ranked_objects(k)
        obj, cls = self.obj_eq[a:b].cpu().numpy() + shift, self.cls_eq[a:b].cpu().numpy()
        obj_color = np.random.RandomState(0).randint(0, 255, (int(obj.max()) + 1, 3))
        lines = []
        for rank, i in enumerate(ranked):
            c = int(cls[np.nonzero(obj == i)[0][0]])
            name = names.get(c, 'class %d' % c)
            if name not in EXCLUDED_FROM_LEGEND:
                lines.append('%s #%d: %d %d %d' % ((name, rank) + tuple(int(v) for v in obj_color[rank + 1])))
        return lines


def main(argv=None):
    ap = argparse.ArgumentParser(description="Rooms of an HDF5 room file as PLY clouds (the reference's h5_to_ply.py)")
    ap.add_argument('file')
    ap.add_argument('--rgb', action='store_true', help='scan colours (default): OUT/rgb/<room>.ply')
    ap.add_argument('--seg', action='store_true', help='ground-truth instances, coloured by their rank in size: OUT/gt/<room>.ply')
    ap.add_argument('--cls', action='store_true', help='class colours from --class-table: OUT/class/<room>.ply')
    ap.add_argument('--target', type=int, default=None, metavar='N', help='print the legend of room N: rank, class and colour of its objects')
    ap.add_argument('--resolution', type=float, default=0.1)
    ap.add_argument('--class-table', default=None, metavar='FILE', help='lines "id name r g b": class names and class colours')
    ap.add_argument('--out', default='data', metavar='DIR', help='output directory, created if absent (default: data)')
    ap.add_argument('--device', default='cuda:0')
    args = ap.parse_args(argv)
    mode = 'target' if args.target is not None else 'cls' if args.cls else 'seg' if args.seg else 'rgb'      # :49-60: the later flag wins
    if mode == 'cls' and args.class_table is None:
        ap.error('--cls needs --class-table FILE (lines "id name r g b"): the class colours are not built in')
    try:
        return _convert(args, mode)
    except ValueError as e:
        ap.error(str(e))


def _convert(args, mode):
    from . import io as lio
    names, colours = ({}, None) if args.class_table is None else read_class_table(args.class_table)
    rf = RoomFile(args.file, args.resolution, args.device, rooms=None if mode != 'target' else [args.target])
    if mode == 'target':
        for ln in rf.legend(0, names):
            print(ln)
        return 0
    if not rf.room_ids:
        return 0
    sub = {'rgb': 'rgb', 'seg': 'gt', 'cls': 'class'}[mode]
    rgb = rf.scan_colours() if mode == 'rgb' else rf.instance_colours() if mode == 'seg' else rf.class_colours(colours)
    os.makedirs(os.path.join(args.out, sub), exist_ok=True)
    files = [os.path.join(args.out, sub, '%d.ply' % r) for r in rf.room_ids]
    lio.save_rooms_ply_device(files, rf.room_slices(rf.xyz()), rf.room_slices(rgb.to(rf.rows.device).contiguous()), device=rf.dev)
    return 0


def examine_main(argv=None):
    ap = argparse.ArgumentParser(description="Datasets of an HDF5 file (the reference's examine_h5.py)")
    ap.add_argument('file')
    examine(ap.parse_args(argv).file)
    return 0
