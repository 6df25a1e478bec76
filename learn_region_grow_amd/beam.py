"""Beam-search region growing (the reference's third local-search driver, test_beam_search.py:143-290) on the same
kernels as the greedy / random-restart loop.

Per seed a queue of at most ``beam_width`` masks; every queue entry spawns ``search_width`` stochastic grow steps; the
children whose mask changed are scored, the best ``beam_width`` form the next queue; the head of the queue is committed when
its bounding box stalls twice or no child survives.  The score is the sort key of every level: ``scoring='np'`` the size of the
child's mask, ``scoring='ml'`` the parent's score plus the log-likelihood of the add / remove masks the child sampled
(test_beam_search.py:237-257,:273; ``lrg_beam_ml_score``, computed on the device between the network and the mask update).  Under
``'ml'`` an emptied mask can hold a place among the best ``beam_width``; it is dropped afterwards and the queue comes out shorter.

All children of a level -- of every room in flight -- are one batch: child ``qid * search_width + search_id`` of a group of ``beam_width * search_width`` slots, its random
stream keyed (seed point, child ordinal, level), so the result does not depend on the order or batching (the reference draws
them one after the other from one stream: that order is the ``rng='legacy'`` definition of the greedy path and is not
offered here).  The queue logic (survivors by score, stall test, commit, next seed, child set-up) runs on the device too
(``lrg_beam_advance``, one workgroup per room): a level is one C call and nothing returns to the host in between.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import LrgBeamGroup, LrgBeamTraceRec
from .grow import RegionGrower, _ptr, _stream_ptr


class BeamSearchGrower(RegionGrower):
    """A room in flight = one group of beam_width * search_width slots; a level of every room in flight = one call of
    lrg_beam_level (queue logic, child set-up, the loop's kernels) with no host decision in between.  The host only watches the
    stats ring for finished rooms (as in greedy growing), fills them in and binds the next room."""
    device_bind = False      # (groups of beam x search slots with a queue of their own: bound on the host, bind_group; reset_room eager)

    def __init__(self, net, rooms_in_flight=16, beam_width=3, search_width=3, seed=0, policy='net', resolution=0.1,
                 cluster_threshold=10, scoring='np', trace=False, trace_capacity=0):
        """scoring: 'np' (mask size) or 'ml' (log-likelihood of the sampled masks), the sort key of every level.
        trace: every RoomResult of run() carries ``beam_trace``, a list of (seed, level, [(child ordinal, mask size, score), ...]) in
        (seed order, level) order: the best beam_width children of each evaluated level before the emptied ones (size 0) are dropped;
        under 'np' the score is the size.  trace_capacity: records of the device buffer (0 = 64 per room in flight, at least 1024); it is
        read out before it can fill, and an overflow raises."""
        if scoring not in ('np', 'ml'):
            raise ValueError(scoring)
        self.beam_width, self.search_width = int(beam_width), int(search_width)
        if not (1 <= self.beam_width <= 16 and 1 <= self.search_width and self.beam_width * self.search_width <= 64):
            raise ValueError('beam_width <= 16 and beam_width * search_width <= 64')
        super().__init__(net, rooms_in_flight=rooms_in_flight, restarts=1, group_size=self.beam_width * self.search_width,
                         rng='counter', seed=seed, policy=policy, resolution=resolution, cluster_threshold=cluster_threshold,
                         packed=False)     # the levels run through lrg_beam_level
        self.cluster_threshold = cluster_threshold
        self.scoring = scoring      # (RegionGrower's own scoring='ml' is the restart score of the packed iteration: not asked for above)
        self.trace = bool(trace)
        self.trace_capacity = int(trace_capacity) if trace_capacity else max(1024, 64 * self.n_groups)
        if self.trace and self.trace_capacity < 2 * self.n_groups:
            raise ValueError('trace_capacity: at least two records per room in flight')

    def enqueue_iteration(self):
        raise _lib.LrgHipError('BeamSearchGrower advances level by level (run()); the lock-step iteration of RegionGrower does not apply')

    enqueue = enqueue_graph = grow_loaded = enqueue_iteration

    def load_rooms(self, rooms):
        self.params.scoring = 0      # (load_rooms refuses the restart score without the packed iteration; the beam's is set below)
        super().load_rooms(rooms)
        self.params.scoring = 1 if self.scoring == 'ml' else 0
        if self.trace:
            self.d_trace = torch.zeros(self.trace_capacity * ctypes.sizeof(LrgBeamTraceRec), dtype=torch.uint8, device=self.dev)
            self.d_trace_count = torch.zeros(1, dtype=torch.int32, device=self.dev)
            self._trace_levels = 0
            self.room_trace = [[] for _ in range(self.n_rooms)]
        self.d_parent = torch.zeros((self.n_groups, self.beam_width, self.cap), dtype=torch.uint8, device=self.dev)
        self.h_groups = (LrgBeamGroup * self.n_groups)()
        for g in range(self.n_groups):
            B = self.h_groups[g]
            B.parent = self.d_parent.data_ptr() + g * self.beam_width * self.cap
            B.cap = self.cap
            B.room = -1
            B.seed = -1
            if self.trace:
                B.trace, B.trace_count, B.trace_cap = self.d_trace.data_ptr(), self.d_trace_count.data_ptr(), self.trace_capacity
        self.d_groups = torch.from_numpy(np.frombuffer(bytes(self.h_groups), dtype=np.uint8).copy()).to(self.dev)
        return self

    def bind_group(self, g, r):
        """Room r (or -1) to group g: the next lrg_beam_advance picks its first seed (:154-156)."""
        B = self.h_groups[g]
        B.room, B.seed, B.pending, B.done = int(r), -1, 0, 0
        B.level = B.stuck = B.steps = B.nq = 0
        sz = ctypes.sizeof(LrgBeamGroup)
        buf = np.frombuffer(bytes(B), dtype=np.uint8).copy()
        self.d_groups[g * sz:(g + 1) * sz].copy_(torch.from_numpy(buf))
        self.group_room[g] = r

    def drain_trace(self):
        """The records written so far, appended to their rooms' lists (a room's records arrive in (seed order, level) order: its group
        writes one per level); the device buffer starts over."""
        count = int(self.d_trace_count.item())
        if count > self.trace_capacity:
            raise _lib.LrgHipError('beam trace overflow: %d records for a buffer of %d' % (count, self.trace_capacity))
        sz = ctypes.sizeof(LrgBeamTraceRec)
        raw = self.d_trace[:count * sz].cpu().numpy().tobytes()
        for k in range(count):
            T = LrgBeamTraceRec.from_buffer_copy(raw, k * sz)
            self.room_trace[T.room].append((int(T.seed), int(T.level), [(int(T.ordinal[i]), int(T.size[i]), float(T.score[i])) for i in range(T.n)]))
        self.d_trace_count.zero_()
        self._trace_levels = 0

    def enqueue_level(self):
        if self.trace:
            if (self._trace_levels + 1) * self.n_groups > self.trace_capacity:      # (a level writes at most one record per group)
                self.drain_trace()
            self._trace_levels += 1
        flags = self.net.forward_flags | (_lib.LRG_FWD_POOL_ZEROED if self.net.mode == 'fused' else 0)
        rc = self.lib.lrg_beam_level(_ptr(self.d_groups), _ptr(self.d_slots), _ptr(self.d_rooms), self.n_groups, self.beam_width,
                                     self.search_width, self.cap, ctypes.byref(self.params), ctypes.byref(self.net._w),
                                     ctypes.byref(self.step_buffers), flags, _stream_ptr(self.dev))
        _lib.check(rc, 'lrg_beam_level')
        self.iterations += 1
        if self.iterations % self.poll_every == 0:
            self._record_poll()

    def run(self, rooms, fill=True):
        """Grow every room once with beam search; RoomResults in input order."""
        with torch.cuda.device(self.dev):
            self.load_rooms(rooms)
            self.reset_state()
            queue = list(range(self.n_rooms))
            for g in range(self.n_groups):
                self.bind_group(g, queue.pop(0) if queue else -1)
            finished = 0
            while finished < self.n_rooms:
                self.enqueue_level()
                for g in self.poll_done():
                    if fill:
                        self.fill(self.group_room[g])
                    finished += 1
                    self.bind_group(g, queue.pop(0) if queue else -1)
            torch.cuda.current_stream(self.dev).synchronize()
            out = self.collect(fill)
            if self.trace:
                self.drain_trace()
                for r, res in enumerate(out):
                    res.beam_trace = self.room_trace[r]
            return out
