"""Training tuples kept on the device, and batches drawn from them there (csrc/lrg_assemble.hip).

``TupleStore`` holds what a staged file holds -- the centred rows of both sides of every tuple with their remove / add flags -- as four flat
device buffers, and per kept tuple the first row and the number of rows of each side.  A tuple's id is its rank among the kept tuples
(``stage.load_staged`` drops the tuples with an empty neighbourhood, train_region_grow.py:128-133; so does ``from_device``, by leaving them
out of the tables: rows are never moved).  ``assemble`` is the job of ``stage.assemble_batch`` (train_region_grow.py:156-175) in two
kernel calls, under the counter stream: the draws of tuple t are ``oracle.rng_ref.CounterStream(rng_seed, t).sample(N, k, purpose,
(0, pass, epoch))``, whatever batch it lands in.  Host twin: tests/assemble_ref.py.

Device memory is what the staged files would hold -- about 4.6 GB for the tuples of 68 Area-5-shaped rooms -- and grows with the areas
loaded; ``concat`` holds its inputs and its result at once.
"""
import ctypes

import numpy as np
import torch

from . import _lib

PASS_TRAIN, PASS_VALIDATION = 0, 1


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


class BatchBuffers:
    """The tensors one assembled batch lives in: inlier [B,Ni,F], neighbor [B,Nn,F] float32, remove [B,Ni], add [B,Nn] int32 and the
    per-instance sums positives_remove [B], positives_add [B] int32."""

    def __init__(self, batch_size, n_inlier, n_neighbor, feature_size, device):
        dev = torch.device(device)
        self.B, self.Ni, self.Nn, self.F = batch_size, n_inlier, n_neighbor, feature_size
        self.inlier = torch.empty((batch_size, n_inlier, feature_size), dtype=torch.float32, device=dev)
        self.neighbor = torch.empty((batch_size, n_neighbor, feature_size), dtype=torch.float32, device=dev)
        self.remove = torch.empty((batch_size, n_inlier), dtype=torch.int32, device=dev)
        self.add = torch.empty((batch_size, n_neighbor), dtype=torch.int32, device=dev)
        self.positives_remove = torch.empty(batch_size, dtype=torch.int32, device=dev)
        self.positives_add = torch.empty(batch_size, dtype=torch.int32, device=dev)


class TupleStore:
    def __init__(self, points, remove, neighbor_points, add, start_in, count_in, start_nb, count_nb, feature_size, rng_seed=0):
        """points [rows,S] / neighbor_points [rows',S] float32 and remove [rows] / add [rows'] int32 device tensors; start_* / count_*: host
        arrays, one entry per kept tuple.  feature_size <= S leading columns make a batch."""
        self.lib = _lib.load()
        self.dev = points.device
        for t, dt in ((points, torch.float32), (neighbor_points, torch.float32), (remove, torch.int32), (add, torch.int32)):
            if t.dtype != dt or not t.is_contiguous() or t.device != self.dev or not t.is_cuda:
                raise ValueError('TupleStore: contiguous float32 rows and int32 flags on one GPU')
        if points.dim() != 2 or neighbor_points.dim() != 2 or points.shape[1] != neighbor_points.shape[1]:
            raise ValueError('TupleStore: rows of both sides as [rows, row_stride]')
        self.points, self.remove, self.neighbor_points, self.add = points, remove, neighbor_points, add
        self.row_stride = int(points.shape[1])
        self.F = int(feature_size)
        if not 1 <= self.F <= self.row_stride:
            raise ValueError('feature_size %d outside 1 .. %d (the stored rows\' width)' % (self.F, self.row_stride))
        self.rng_seed = int(rng_seed) & 0xFFFFFFFF
        self.start_in, self.count_in = np.asarray(start_in, dtype=np.int64), np.asarray(count_in, dtype=np.int32)
        self.start_nb, self.count_nb = np.asarray(start_nb, dtype=np.int64), np.asarray(count_nb, dtype=np.int32)
        T = len(self.start_in)
        if not (len(self.count_in) == len(self.start_nb) == len(self.count_nb) == T):
            raise ValueError('TupleStore: one table entry per tuple and side')
        for start, count, rows, lab in ((self.start_in, self.count_in, points, remove), (self.start_nb, self.count_nb, neighbor_points, add)):
            if rows.shape[0] != lab.shape[0]:
                raise ValueError('TupleStore: one flag per row')
            if T and (count.min() < 1 or start.min() < 0 or (start + count).max() > rows.shape[0]):
                raise ValueError('TupleStore: every kept tuple has at least one row on each side, inside the buffers')
        self._tables = [torch.from_numpy(a.copy()).to(self.dev) for a in (self.start_in, self.count_in, self.start_nb, self.count_nb)]

    def __len__(self):
        return len(self.start_in)

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.points, self.remove, self.neighbor_points, self.add))

    # ---- construction ----
    @classmethod
    def from_staged(cls, data, feature_size=13, device='cuda:0', rng_seed=0):
        """data: what stage.load_staged returns (per-tuple arrays, empty neighbourhoods already dropped).  One upload per buffer."""
        dev = torch.device(device)
        F = int(feature_size)
        if any(len(q) == 0 for q in data['neighbor_points']):
            raise ValueError('from_staged: a tuple with an empty neighbourhood (stage.load_staged drops them)')

        def flat(rows, flags):
            cnt = np.array([len(p) for p in rows], dtype=np.int64)
            if len(rows):
                x = np.ascontiguousarray(np.vstack(rows), dtype=np.float32)
                y = np.ascontiguousarray(np.concatenate(flags), dtype=np.int32)
            else:
                x, y = np.zeros((0, F), np.float32), np.zeros(0, np.int32)
            start = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64) if len(cnt) else np.zeros(0, np.int64)
            return torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), start, cnt.astype(np.int32)
        p, r, s_in, c_in = flat(data['points'], data['remove'])
        q, a, s_nb, c_nb = flat(data['neighbor_points'], data['add'])
        return cls(p, r, q, a, s_in, c_in, s_nb, c_nb, F, rng_seed)

    @classmethod
    def from_device(cls, left, feature_size=13, rng_seed=0):
        """left: the 'device' entry of stage.stage_rooms_gpu(..., download=False).  The tuples with an empty neighbourhood are left out of
        the tables (their inlier rows stay where they are, unused)."""
        row_in, row_nb = np.asarray(left['row_in'], dtype=np.int64), np.asarray(left['row_nb'], dtype=np.int64)
        cnt_in, cnt_nb = np.diff(row_in), np.diff(row_nb)
        keep = np.nonzero(cnt_nb > 0)[0]
        return cls(left['points'], left['remove'], left['neighbor_points'], left['add'], row_in[:-1][keep], cnt_in[keep], row_nb[:-1][keep],
                   cnt_nb[keep], feature_size, rng_seed)

    @classmethod
    def concat(cls, stores):
        """The tuples of several stores (areas) as one, in the order given: ids continue from one store into the next."""
        stores = list(stores)
        if len(stores) == 1:
            return stores[0]
        if not stores or len({(s.row_stride, s.F, s.rng_seed, s.dev) for s in stores}) != 1:
            raise ValueError('concat: stores of one row width, feature size, seed and device')
        off_in = np.concatenate([[0], np.cumsum([s.points.shape[0] for s in stores])])
        off_nb = np.concatenate([[0], np.cumsum([s.neighbor_points.shape[0] for s in stores])])
        return cls(torch.cat([s.points for s in stores]), torch.cat([s.remove for s in stores]), torch.cat([s.neighbor_points for s in stores]),
                   torch.cat([s.add for s in stores]),
                   np.concatenate([s.start_in + off_in[i] for i, s in enumerate(stores)]), np.concatenate([s.count_in for s in stores]),
                   np.concatenate([s.start_nb + off_nb[i] for i, s in enumerate(stores)]), np.concatenate([s.count_nb for s in stores]),
                   stores[0].F, stores[0].rng_seed)

    # ---- batches ----
    def upload_order(self, order):
        """An epoch's tuple order (host integers, each an id of this store) as the int32 device tensor `assemble` slices its batches from."""
        order = np.asarray(order)
        if order.ndim != 1 or (len(order) and (order.min() < 0 or order.max() >= len(self))):
            raise ValueError('order: tuple ids 0 .. %d' % (len(self) - 1))
        return torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).to(self.dev)

    def assemble(self, order, epoch, pass_, out):
        """order: int32 device tensor [B] of tuple ids (a slice of upload_order's result; ids in range are the caller's contract);
        out: BatchBuffers.  Two kernel calls on the current stream; nothing is read back."""
        if order.dtype != torch.int32 or not order.is_contiguous() or order.device != self.dev or order.numel() != out.B:
            raise ValueError('assemble: order must be %d contiguous int32 tuple ids on %s' % (out.B, self.dev))
        if out.F != self.F or out.inlier.device != self.dev:
            raise ValueError('assemble: batch buffers of feature size %d on %s' % (self.F, self.dev))
        t_sin, t_cin, t_snb, t_cnb = self._tables
        with torch.cuda.device(self.dev):
            st = ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
            for rows, lab, start, count, k, purpose, o_rows, o_lab, o_pos in (
                    (self.points, self.remove, t_sin, t_cin, out.Ni, _lib.LRG_PURPOSE_TRAIN_INLIER, out.inlier, out.remove, out.positives_remove),
                    (self.neighbor_points, self.add, t_snb, t_cnb, out.Nn, _lib.LRG_PURPOSE_TRAIN_NEIGHBOR, out.neighbor, out.add, out.positives_add)):
                _lib.check(self.lib.lrg_train_assemble(_ptr(rows), self.row_stride, _ptr(lab), _ptr(start), _ptr(count), _ptr(order), out.B, k, self.F,
                                                       self.rng_seed, int(epoch), int(pass_), purpose, _ptr(o_rows), _ptr(o_lab), _ptr(o_pos), st),
                           'lrg_train_assemble')
        return out
