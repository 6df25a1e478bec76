"""GrowthTrace -- what a grower did to one room, step by step (the state animate_region_growing.py draws: :365-373,:398-401,:403).

One slot group grows the room through the counter stream's lock-step packed iteration, one host call per step; behind each call
lrg_trace_snapshot (csrc/lrg_trace.hip) reads the slot and the room ON THE DEVICE and keeps, per evaluated step, a header (seed, 1-based
step, next_cluster_id, the four counts over the raw points) and a code byte per equalised point (bit 0 before, bit 1 neighbour, bit 2
after), plus the running `paint` of the seg frames.  The host synchronises once per batch of `frames_per_batch` calls.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .lrgnet import _ptr, _stream_ptr

HEADER_WORDS = 8
HEADER_FIELDS = ('seed', 'step', 'cluster_id', 'inlier', 'neighbor', 'add', 'remove')
ERRORS = {1: 'a step without a successor', 2: 'a list entry outside the room', 4: 'the frame ring is full', 8: 'not the room the buffers were sized for'}


class TraceBatch:
    """The frames completed by one batch of host calls: headers [k, 8] int32 (host), codes / paints [k, stride] uint8 (device)."""

    def __init__(self, first, headers, codes, paints):
        self.first, self.headers, self.codes, self.paints = first, headers, codes, paints

    def __len__(self):
        return len(self.headers)


def make_grower(net, seed=0, policy='net', resolution=0.1, **kw):
    """The grower a trace drives: one room in flight, greedy growing, counter stream, lock-step packed iterations."""
    from .grow import RegionGrower
    return RegionGrower(net, rooms_in_flight=1, restarts=1, rng='counter', seed=seed, policy=policy, resolution=resolution, packed=True,
                        free_run=False, **kw)


class GrowthTrace:
    def __init__(self, grower, room, unequalized_idx=None, frames_per_batch=16):
        """room: dict of points [n, F], obj_id [n], order [n], room_id (RegionGrower.load_rooms); unequalized_idx [M]: the equalised point of
        every raw point (preprocess_room; default: the room's points are the raw points)."""
        gr = self.gr = grower
        if gr.rng != 'counter':
            raise ValueError("GrowthTrace reads the state a packed iteration leaves behind; rng='legacy' takes the nine-launch step, which ends "
                             'behind the mask update and leaves a different state: use the counter stream')
        if gr.params.restarts != 1 or gr.G != 1 or gr.speculate or getattr(gr, 'beam_width', 0):
            raise ValueError('GrowthTrace follows greedy growing only (restarts = 1, no beam, no speculation)')
        if frames_per_batch < 1:
            raise ValueError('frames_per_batch must be at least 1')
        self.B = int(frames_per_batch)
        with torch.cuda.device(gr.dev):
            gr.load_rooms([room])
            if not gr.packed or gr.free_run:
                raise ValueError('GrowthTrace needs lock-step packed iterations (RegionGrower(packed=True, free_run=False), rooms of at most %d points)'
                                 % _lib.LRG_PACKED_MAX_POINTS)
            n = self.n = gr.room_n[0]
            assert gr.cap % 16 == 0 and int(gr.room_off[0]) % 16 == 0      # (the snapshot reads masks and flags a word at a time)
            self.stride = (n + 15) // 16 * 16
            self.cap = self.B + 1                                            # the frame still open from the batch before, and one per call
            dev = gr.dev
            uneq = np.arange(n) if unequalized_idx is None else np.asarray(unequalized_idx)
            if len(uneq) and (uneq.min() < 0 or uneq.max() >= n):
                raise ValueError('unequalized_idx names points outside the room')
            mult = np.zeros(self.stride, dtype=np.int32)
            mult[:n] = np.bincount(uneq, minlength=n)
            self.d_mult = torch.from_numpy(mult).to(dev)
            self.d_state = torch.zeros(8, dtype=torch.int32, device=dev)
            self.d_plan = torch.zeros(8, dtype=torch.int32, device=dev)
            self.d_headers = torch.zeros((self.cap, HEADER_WORDS), dtype=torch.int32, device=dev)
            self.d_codes = torch.zeros((self.cap, self.stride), dtype=torch.uint8, device=dev)
            self.d_paints = torch.zeros((self.cap, self.stride), dtype=torch.uint8, device=dev)
            self.d_paint = torch.zeros(self.stride, dtype=torch.uint8, device=dev)
            self.d_visprev = torch.zeros(self.stride, dtype=torch.uint8, device=dev)
            self.d_mark = torch.zeros(self.stride, dtype=torch.uint8, device=dev)
            self.h_state = torch.zeros(8, dtype=torch.int32).pin_memory()
            self.h_headers = torch.zeros((self.cap, HEADER_WORDS), dtype=torch.int32).pin_memory()
            self.h_stats = torch.zeros(2, dtype=torch.int64).pin_memory()
            gr.reset_state()
            self._done_base = gr._seen_done
            gr.bind(0, 0)
        self.consumed = 0
        self.calls = 0
        self.finished = False

    def snapshot(self):
        gr = self.gr
        _lib.check(gr.lib.lrg_trace_snapshot(_ptr(gr.d_slots), _ptr(gr.d_rooms), 0, 0, self.n, self.stride, self.cap, self.consumed,
                                             _ptr(self.d_state), _ptr(self.d_plan), _ptr(self.d_headers), _ptr(self.d_codes), _ptr(self.d_paints),
                                             _ptr(self.d_paint), _ptr(self.d_visprev), _ptr(self.d_mark), _ptr(self.d_mult), _stream_ptr(gr.dev)),
                   'lrg_trace_snapshot')

    def step(self):
        """One packed iteration and its snapshot, enqueued: no host synchronisation."""
        self.gr.enqueue_iteration()
        self.snapshot()
        self.calls += 1

    def next_batch(self):
        """frames_per_batch steps, one synchronisation, the frames they completed (possibly none).  None once the room is finished and every frame taken."""
        if self.finished:
            return None
        gr = self.gr
        with torch.cuda.device(gr.dev):
            for _ in range(self.B):
                self.step()
            self.h_state.copy_(self.d_state, non_blocking=True)
            self.h_headers.copy_(self.d_headers, non_blocking=True)
            self.h_stats.copy_(gr.d_stats[:2], non_blocking=True)
            torch.cuda.current_stream(gr.dev).synchronize()
            frames, pending, _, err, done = [int(x) for x in self.h_state[:5]]
            if err:
                raise _lib.LrgHipError('lrg_trace_snapshot: ' + ', '.join(msg for bit, msg in ERRORS.items() if err & bit))
            assert done == frames - pending and self.consumed <= done <= self.consumed + self.cap
            rows = [f % self.cap for f in range(self.consumed, done)]
            headers = self.h_headers.numpy()[rows].copy()
            assert (headers[:, 7] == 1).all()
            sel = torch.tensor(rows, dtype=torch.int64, device=gr.dev)
            batch = TraceBatch(self.consumed, headers, self.d_codes.index_select(0, sel), self.d_paints.index_select(0, sel))
            self.consumed = done
            if int(self.h_stats[1]) > self._done_base and not pending:
                self.finished = True
        return batch

    def batches(self):
        while True:
            b = self.next_batch()
            if b is None:
                return
            if len(b):
                yield b

    def result(self, fill=True):
        """The room's RoomResult, as RegionGrower.run returns it (call once the trace is finished)."""
        gr = self.gr
        if not self.finished:
            raise ValueError('the room is not finished')
        with torch.cuda.device(gr.dev):
            if fill:
                gr.fill(0)
            torch.cuda.current_stream(gr.dev).synchronize()
            return gr.collect(fill)[0]
