"""Step audit: what a grower holds on the device after ONE host call, against the oracle hook's record of the same step.

grow_ref.grow_room(hook=...) yields one record per evaluated step.  A packed iteration (lrg_grow_step_packed) and a free-running
launch of one step (lrg_grow_async) end every slot between the evaluation and the mask update, so each ACTIVE slot then describes
exactly the record (slot.seed, slot.restart, slot.step).  The nine-launch step (lrg_grow_step) ends with lrg_mask_update: there an
ACTIVE slot describes the record (seed, restart, step - 1), and its mask is the one the NEXT record starts from.

`expected` turns a record into the device quantities, `compare` checks a device state against them BIT FOR BIT (floats by their bit
patterns: no tolerance anywhere), `read_state` reads a slot's state from a RegionGrower, `Audit` drives a whole run.  The first three
are NumPy only, so that the comparer itself is tested on the host with planted faults (test_median_rooms_host.py)."""

import numpy as np

from oracle import grow_ref, rng_ref

FORMS = ('greedy', 'general', 'free', 'step')
# what a formulation leaves behind -- and the audit insists on finding:
#   greedy   lrg_front_greedy_kernel + lrg_front_big_kernel: UNCENTRED packed rows (the network subtracts the centre while staging them) and no
#            sample positions -- the kernel never stores them, its mask update draws them again from the counter stream; the positions of the
#            distinct rows are pinned all the same by the rows themselves (a room's points are distinct)
#   general  lrg_front_kernel<7> / <1> + <4>: centred packed rows, sample positions
#   free     lrg_grow_async: the greedy front, rows of the slot's own at a 64-byte stride
#   step     lrg_grow_step: padded per-slot sets, ground-truth flags per sample slot
REQUIRED = {
    'greedy': ('slot', 'mask', 'cur_list', 'cand_list', 'center', 'slot_rows', 'x_in', 'x_nb', 'upd_in', 'upd_nb'),
    'general': ('slot', 'mask', 'cur_list', 'cand_list', 'center', 'sample_in', 'sample_nb', 'slot_rows', 'x_in', 'x_nb', 'upd_in', 'upd_nb'),
    'free': ('slot', 'mask', 'cur_list', 'cand_list', 'center', 'slot_rows', 'x_in', 'x_nb', 'upd_in', 'upd_nb'),
    'step': ('slot', 'cur_list', 'cand_list', 'center', 'sample_in', 'sample_nb', 'inlier', 'neighbor', 'gt_remove', 'gt_add'),
}
CENTRED_ROWS = {'greedy': False, 'general': True, 'free': False}


def zero_net(Ni=512, Nn=512):
    def fn(xi, xn):
        return np.zeros((1, Nn, 2), np.float32), np.zeros((1, Ni, 2), np.float32)
    return fn


def slim(h):
    """The part of a hook record the audit reads, masks packed to bits (a 98 k-point room takes 500 steps)."""
    return dict(seed=h['seed'], restart=h['restart'], step=h['step'], nc=h['nc'], ne=h['ne'], center=h['center'],
                subset_in=h['subset_in'], subset_nb=h['subset_nb'], inlier=h['inlier'][0], neighbor=h['neighbor'][0],
                add=h['add'][0], rmv=h['rmv'][0], input_add=h['input_add'], input_remove=h['input_remove'],
                n=len(h['mask_before']), mask_bits=np.packbits(h['mask_before']), visited_bits=np.packbits(h['visited']),
                min_dims=h['min_dims'], max_dims=h['max_dims'])


def oracle_run(room, seed, policy='gt', net_fn=None, Ni=512, Nn=512, restarts=0, resolution=0.1):
    """-> (GrowResult, {(seed point, restart, step): slim record}) of one room under the counter stream."""
    recs = {}

    def hook(h):
        key = (h['seed'], h['restart'], h['step'])
        assert key not in recs
        recs[key] = slim(h)
    want = grow_ref.grow_room(room['points'], room['obj_id'], room['order'], None, rng_ref.CounterStream(seed, room['room_id']),
                              net_fn=net_fn or zero_net(Ni, Nn), policy=policy, num_inlier=Ni, num_neighbor=Nn, restarts=restarts,
                              resolution=resolution, hook=hook)
    return want, recs


def mask_of(rec, which='mask_bits'):
    return np.unpackbits(rec[which], count=rec['n']).astype(bool)


def expected(room, rec, Ni=512, Nn=512, voxels=None, resolution=0.1):
    """The device quantities of one step, from its record and the room alone."""
    pts = room['points']
    F = pts.shape[1]
    pv = grow_ref.voxelize(pts[:, :3], resolution) if voxels is None else voxels
    mask, visited = mask_of(rec), mask_of(rec, 'visited_bits')
    cur = np.flatnonzero(mask)
    # the dilated-box candidates in index order (test_region_grow.py:221-229), restated from the record's box and visited flags
    box = np.all(pv >= rec['min_dims'] - 1, axis=1) & np.all(pv <= rec['max_dims'] + 1, axis=1)
    cand = np.flatnonzero(box & ~mask & ~visited)
    nc, ne = rec['nc'], rec['ne']
    assert len(cur) == nc and len(cand) == ne
    rin, rnb = min(nc, Ni), min(ne, Nn)
    center = np.zeros(16, np.float32)
    cch = [c for c in range(F) if c < 2 or c >= 6]
    center[cch] = rec['center'][cch]
    src_in, src_nb = cur[rec['subset_in'][:rin]], cand[rec['subset_nb'][:rnb]]
    # (the leading rows of a stacked set are its distinct ones: a padded set's members in order, a full set's whole draw, :237-240)
    assert len(set(src_in.tolist())) == rin and len(set(src_nb.tolist())) == rnb
    return dict(slot=dict(nc=nc, ne=ne, mn=[int(x) for x in rec['min_dims']], mx=[int(x) for x in rec['max_dims']],
                          target=int(room['obj_id'][rec['seed']])),
                mask=mask, cur_list=cur, cand_list=cand, center=center,
                sample_in=np.asarray(rec['subset_in']), sample_nb=np.asarray(rec['subset_nb']),
                rows=(rin, rnb), x_in_centred=rec['inlier'][:rin], x_nb_centred=rec['neighbor'][:rnb],
                x_in_raw=pts[src_in], x_nb_raw=pts[src_nb],
                flag_in=rec['input_remove'][:rin].astype(np.float32), flag_nb=rec['input_add'][:rnb].astype(np.float32),
                rmv_logits=rec['rmv'][:rin], add_logits=rec['add'][:rnb],
                inlier=rec['inlier'], neighbor=rec['neighbor'], gt_remove=np.asarray(rec['input_remove']), gt_add=np.asarray(rec['input_add']))


def perfect_state(exp, form, logits=False):
    """The state a correct device would hold (the host test plants its faults in a copy of this)."""
    rin, rnb = exp['rows']
    st = dict(slot=dict(exp['slot'], mn=list(exp['slot']['mn']), mx=list(exp['slot']['mx'])), mask=exp['mask'].copy(),
              cur_list=exp['cur_list'].astype(np.int32), cand_list=exp['cand_list'].astype(np.int32), center=exp['center'].copy())
    if form in ('general', 'step'):
        st['sample_in'], st['sample_nb'] = exp['sample_in'].astype(np.int32), exp['sample_nb'].astype(np.int32)
    if form == 'step':
        st.update(inlier=exp['inlier'].copy(), neighbor=exp['neighbor'].copy(), gt_remove=exp['gt_remove'].astype(np.int32),
                  gt_add=exp['gt_add'].astype(np.int32))
        del st['mask']
        return st
    kind = 'centred' if CENTRED_ROWS[form] else 'raw'
    st.update(slot_rows=np.array([rin, rnb, 0, 0], np.int32), x_in=exp['x_in_' + kind].copy(), x_nb=exp['x_nb_' + kind].copy())
    for side, rows, flag in (('in', st['x_in'], exp['flag_in']), ('nb', st['x_nb'], exp['flag_nb'])):
        st['upd_' + side] = np.concatenate([rows[:, :3], flag[:, None]], axis=1).astype(np.float32)
    if logits:
        st['rmv_logits'], st['add_logits'] = exp['rmv_logits'].copy(), exp['add_logits'].copy()
    return st


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(name, got, want, ctx):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, '%s: %s has shape %s, the oracle %s' % (ctx, name, got.shape, want.shape)
    if want.dtype == np.float32:
        assert got.dtype == np.float32, '%s: %s is %s' % (ctx, name, got.dtype)
    bad = np.flatnonzero((_bits(got) != _bits(want)).reshape(-1))
    if len(bad):
        i = int(bad[0])
        raise AssertionError('%s: %s differs from the oracle at %d of %d elements, first at flat index %d: %r against %r'
                             % (ctx, name, len(bad), want.size, i, got.reshape(-1)[i], want.reshape(-1)[i]))


def compare(state, exp, form, ctx='', logits=False, mask_after=None):
    """Raises AssertionError unless `state` (a device state, or perfect_state's model of one) is the oracle's step `exp`, bit for bit.
    mask_after (form 'step' only): the mask the next record of the region starts from, when there is one."""
    need = REQUIRED[form] + (('rmv_logits', 'add_logits') if logits else ())
    missing = [k for k in need if k not in state]
    assert not missing, '%s: the %s form left no %s to audit' % (ctx, form, missing)
    sl, want = state['slot'], exp['slot']
    for k in ('nc', 'ne', 'target'):
        assert int(sl[k]) == int(want[k]), '%s: slot.%s = %d, the oracle has %d' % (ctx, k, sl[k], want[k])
    for k in ('mn', 'mx'):
        assert [int(x) for x in sl[k]] == want[k], '%s: slot.%s = %s, the oracle has %s' % (ctx, k, list(sl[k]), want[k])
    if form == 'step':
        if mask_after is not None:
            _same('mask after the update', state['mask'], mask_after, ctx)
    else:
        _same('mask', state['mask'], exp['mask'], ctx)
    _same('current list', state['cur_list'], exp['cur_list'].astype(np.int32), ctx)
    _same('candidate list', state['cand_list'], exp['cand_list'].astype(np.int32), ctx)
    _same('centre', state['center'], exp['center'], ctx)
    if 'sample_in' in need:
        _same('inlier sample positions', state['sample_in'], exp['sample_in'].astype(np.int32), ctx)
        _same('neighbour sample positions', state['sample_nb'], exp['sample_nb'].astype(np.int32), ctx)
    if form == 'step':
        _same('inlier set', state['inlier'], exp['inlier'], ctx)
        _same('neighbour set', state['neighbor'], exp['neighbor'], ctx)
        _same('input_remove', state['gt_remove'], exp['gt_remove'].astype(np.int32), ctx)
        _same('input_add', state['gt_add'], exp['gt_add'].astype(np.int32), ctx)
        return
    rin, rnb = exp['rows']
    assert [int(x) for x in state['slot_rows'][:2]] == [rin, rnb], '%s: slot_rows = %s, the oracle has %d / %d distinct rows' % (ctx, list(state['slot_rows']), rin, rnb)
    kind = 'centred' if CENTRED_ROWS[form] else 'raw'
    for side, flag in (('in', exp['flag_in']), ('nb', exp['flag_nb'])):
        rows = exp['x_%s_%s' % (side, kind)]
        _same('packed %s rows (%s)' % ('inlier' if side == 'in' else 'neighbour', 'centred' if kind == 'centred' else 'uncentred'), state['x_' + side], rows, ctx)
        if kind == 'raw':      # uncentred plus the centre IS the oracle's row (:243-247)
            F = rows.shape[1]
            _same('packed %s rows minus the centre' % side, state['x_' + side] - state['center'][None, :F], exp['x_%s_centred' % side], ctx)
        _same('upd_%s columns 0..2' % side, state['upd_' + side][:, :3], rows[:, :3], ctx)
        _same('upd_%s column 3 (%s)' % (side, 'input_remove' if side == 'in' else 'input_add'), state['upd_' + side][:, 3], flag, ctx)
    if logits:
        _same('remove logits', state['rmv_logits'], exp['rmv_logits'], ctx)
        _same('add logits', state['add_logits'], exp['add_logits'], ctx)


# ---------------------------------------------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------------------------------------------
class Snapshot:
    """The small per-call arrays of a grower, read once for all its slots."""

    def __init__(self, gr, form):
        self.slots = gr._read_slots()
        self.center = gr.b_center.cpu().numpy()
        if form in ('general', 'step'):
            self.sample_in, self.sample_nb = gr.b_sin.cpu().numpy(), gr.b_snb.cpu().numpy()
        if form != 'step':
            self.slot_rows = gr.p_slot_rows.cpu().numpy()


def read_state(gr, snap, s, form, logits=False):
    """Slot s of grower gr after a host call (the stream synchronised by the caller)."""
    sl = snap.slots[s]
    n, nc, ne = gr.room_n[sl.room], sl.nc, sl.ne
    F, Ni, Nn = gr.net.feature_size, gr.net.num_inlier_points, gr.net.num_neighbor_points
    st = dict(slot=dict(nc=nc, ne=ne, mn=list(sl.mn), mx=list(sl.mx), target=sl.target),
              mask=gr.d_cur[s, :n].cpu().numpy().astype(bool),
              cur_list=gr.d_curidx[s, :nc].cpu().numpy(), cand_list=gr.d_candidx[s, :ne].cpu().numpy(), center=snap.center[s].copy())
    if form in ('general', 'step'):
        st['sample_in'], st['sample_nb'] = snap.sample_in[s], snap.sample_nb[s]
    if form == 'step':
        st.update(inlier=gr.b_inl[s].cpu().numpy(), neighbor=gr.b_nbr[s].cpu().numpy(), gt_remove=gr.b_gtr[s].cpu().numpy(),
                  gt_add=gr.b_gta[s].cpu().numpy())
        return st
    rin, rnb, oi, on = [int(x) for x in snap.slot_rows[s]]
    st['slot_rows'] = snap.slot_rows[s]
    assert 0 <= rin <= Ni and 0 <= rnb <= Nn and 0 <= oi and 0 <= on and oi + rin <= gr.row_cap and on + rnb <= gr.row_cap, (s, snap.slot_rows[s])
    stride = F
    if form == 'free':
        assert gr.async_buffers.rows16 == 1 and not gr.tail_rows      # rows of the slot's own, 16 floats apart
        stride = 16
    for side, buf, o, r in (('in', gr.p_xin, oi, rin), ('nb', gr.p_xnb, on, rnb)):
        rows = buf.view(-1)[o * stride:(o + r) * stride].cpu().numpy().reshape(r, stride)
        if stride > F:
            assert not rows[:, F:].any(), 'slot %d: columns past the features are not zero' % s
        st['x_' + side] = np.ascontiguousarray(rows[:, :F])
    st['upd_in'], st['upd_nb'] = gr.p_updin[s, :rin].cpu().numpy(), gr.p_updnb[s, :rnb].cpu().numpy()
    if logits:
        st['rmv_logits'], st['add_logits'] = gr.p_rmv[oi:oi + rin].cpu().numpy(), gr.p_add[on:on + rnb].cpu().numpy()
    return st


def form_of(gr):
    """The formulation a loaded grower runs, as the library itself decides it."""
    import ctypes
    if gr.free_run:
        return 'free'
    if not gr.packed:
        return 'step'
    # (uncentred rows plus a centre array: the greedy front -- include/lrg_hip.h, lrg_packed_rows_center)
    return 'greedy' if gr.lib.lrg_packed_rows_center(ctypes.byref(gr.params), ctypes.byref(gr.packed_buffers)) else 'general'


class Audit:
    """One audited run: the rooms bound by hand, one slot group each, then one host call at a time."""

    def __init__(self, gr, rooms, oracles, form, logits=False, every_record=True):
        """oracles: per room (GrowResult, records) of oracle_run.  every_record: every oracle record must be met (a host call = one
        step per slot); False: a host call takes several steps (HIP-graph replay), the records met are a subset."""
        import torch
        from learn_region_grow_amd._lib import LRG_ACTIVE
        self.torch, self.ACTIVE = torch, LRG_ACTIVE
        assert form in FORMS
        self.gr, self.rooms, self.oracles, self.form, self.logits, self.every_record = gr, rooms, oracles, form, logits, every_record
        self.voxels = [grow_ref.voxelize(r['points'][:, :3], gr.params.resolution) for r in rooms]
        self.seen = [set() for _ in rooms]
        self.calls = 0
        gr.load_rooms(rooms)
        # (more slot groups than rooms: the rest are bound to no room, as RegionGrower.bind_first leaves them, and check() walks the ACTIVE slots only --
        #  the slot count decides the shape of a free-running launch, so a launch of many slots can be audited on a few rooms)
        assert gr.n_groups >= len(rooms) and form_of(gr) == form, (form_of(gr), form)
        gr.reset_state()
        for g in range(gr.n_groups):
            gr.bind(g, g if g < len(rooms) else -1)

    def check(self):
        """Every ACTIVE slot against its record."""
        gr, form = self.gr, self.form
        self.torch.cuda.current_stream(gr.dev).synchronize()
        snap = Snapshot(gr, form)
        taken = []          # packed rows of the ACTIVE slots: no two slots share a row
        for s in range(gr.S):
            sl = snap.slots[s]
            if sl.status != self.ACTIVE or sl.room < 0:
                continue
            r = sl.room
            step = sl.step - 1 if form == 'step' else sl.step
            key = (sl.seed, sl.restart, step)
            ctx = 'call %d, slot %d, room %d, seed %d restart %d step %d (nc %d)' % (self.calls, s, r, sl.seed, sl.restart, step, sl.nc)
            recs = self.oracles[r][1]
            assert key in recs, '%s: the oracle evaluated no such step' % ctx
            assert key not in self.seen[r], '%s: seen twice' % ctx
            self.seen[r].add(key)
            Ni, Nn = gr.net.num_inlier_points, gr.net.num_neighbor_points
            exp = expected(self.rooms[r], recs[key], Ni, Nn, voxels=self.voxels[r], resolution=gr.params.resolution)
            nxt = recs.get((key[0], key[1], key[2] + 1))
            compare(read_state(gr, snap, s, form, self.logits), exp, form, ctx, self.logits, mask_after=mask_of(nxt) if nxt else None)
            if form != 'step':
                rin, rnb, oi, on = [int(x) for x in snap.slot_rows[s]]
                for a, b, oa, ob in taken:
                    assert (oi + rin <= oa or oa + a <= oi) and (on + rnb <= ob or ob + b <= on), '%s: packed rows overlap another slot\'s' % ctx
                taken.append((rin, rnb, oi, on))

    def run(self, call, max_calls=100000):
        """call(): one host call.  Until every room is finished; then the records and labels against the oracle's."""
        gr = self.gr
        while True:
            call()
            self.calls += 1
            self.check()
            if int(gr.d_stats[1].item()) >= len(self.rooms):
                break
            assert self.calls < max_calls
        for r in range(len(self.rooms)):
            gr.fill(r)
        self.torch.cuda.current_stream(gr.dev).synchronize()
        res = gr.collect()
        print('step audit (%s): %d steps of %d met in %d host calls' % (self.form, sum(len(x) for x in self.seen), sum(len(o[1]) for o in self.oracles), self.calls))
        key = lambda x: (x['seed'], x['steps'], x['points'], x['reason'], x['labeled'])
        for r, (want, recs) in enumerate(self.oracles):
            if self.every_record:
                missed = sorted(set(recs) - self.seen[r])
                assert not missed, 'room %d: %d oracle steps never seen on the device, first %s' % (r, len(missed), missed[0])
            assert self.seen[r] <= set(recs) and self.seen[r]
            assert [key(x) for x in res[r].regions] == [key(x) for x in want.regions]
            np.testing.assert_array_equal(res[r].cluster_label, want.cluster_label)
            np.testing.assert_array_equal(res[r].filled_label, want.filled_label)
        return res
