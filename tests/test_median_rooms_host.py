"""Host: the rooms of median_rooms.py do what the GPU step audit relies on, and the audit's comparer catches planted faults -- so that
test_gpu_step_audit.py cannot pass for the wrong reason.  Oracle only (ground-truth masks, a zero network): no GPU."""
import numpy as np
import pytest

import median_rooms as mr
import step_audit as sa
from oracle import grow_ref

SEED = 5


@pytest.fixture(scope='module')
def classes():
    room = mr.classes_room()
    return (room,) + sa.oracle_run(room, SEED)


@pytest.fixture(scope='module')
def big():
    room = mr.big_room()
    return (room,) + sa.oracle_run(room, SEED)


@pytest.fixture(scope='module')
def even():
    room = mr.even_room()
    return (room,) + sa.oracle_run(room, SEED)


@pytest.mark.parametrize('make,kw,n', [(mr.even_room, {}, 49667), (mr.even_room, dict(wide=True), 49668),
                                       (mr.classes_room, {}, 43548), (mr.classes_room, dict(wide=True), 43548), (mr.classes_room, dict(F=12), 43548),
                                       (mr.cut_room, {}, 10773), (mr.big_room, {}, 98311), (mr.big_room, dict(wide=True), 98311)])
def test_voxels_are_unique(make, kw, n):
    room = make(**kw)
    assert room['points'].shape == (n, kw.get('F', 13)) and room['points'].dtype == np.float32
    v = grow_ref.voxelize(room['points'][:, :3], mr.RES)
    assert len(np.unique(grow_ref.pack_voxels(v))) == n
    extent = v.max(axis=0) - v.min(axis=0)
    assert (extent[1] > 2047) == bool(kw.get('wide'))          # packed voxel words hold 2048 x 2048 x 1024 voxels
    assert extent[0] <= 2047 and extent[2] == 0
    assert sorted(room['order'].tolist()) == list(range(n))
    assert room['order'][:len(room['strips'])].tolist() == [f for f, _, _ in room['strips']]      # the corners are the first seeds


def _regions_fill_their_strips(room, want, recs, steps, max_ne):
    strips = room['strips']
    assert want.total_steps == len(recs) == steps
    assert max(r['ne'] for r in recs.values()) == max_ne <= 512
    for (first, W, count), reg in zip(strips, want.regions):
        # square growth from the corner until the strip's width or length is exhausted, then line by line; one more step at the full size
        assert (reg['seed'], reg['points'], reg['reason'], reg['labeled']) == (first, count, 'noexpand', True), reg
        assert reg['steps'] == max(W, -(-count // W))
        last = recs[(first, 0, reg['steps'] - 1)]
        assert last['nc'] == count and last['ne'] == 3         # the median IS taken at the full size: only the fence is on offer
    for reg in want.regions[len(strips):]:                     # the fences: three points, two steps, never labelled
        assert reg['points'] == 3 and reg['steps'] == 2 and not reg['labeled']
    assert len(want.regions) == 2 * len(strips)


def test_classes_room_stops_at_the_boundaries(classes):
    room, want, recs = classes
    _regions_fill_their_strips(room, want, recs, 500, 255)
    assert [r['steps'] for r in want.regions[:8]] == [16, 17, 32, 33, 64, 65, 128, 129]


def test_big_room_stops_at_the_boundaries(big):
    room, want, recs = big
    _regions_fill_their_strips(room, want, recs, 516, 383)
    assert [r['steps'] for r in want.regions[:2]] == [256, 256]


def test_even_room_stops_at_its_size(even):
    room, want, recs = even
    _regions_fill_their_strips(room, want, recs, 258, 387)
    ncs = sorted(r['nc'] for r in recs.values())
    assert [nc for nc in ncs if nc > 49152] == [49276, 49470, 49664]
    # the square phase alternates (k * k up to 194 * 194), the lines after it are all even
    assert all(nc % 2 == 0 for nc in ncs if nc >= 194 * 194) and sum(1 for nc in ncs if 16384 < nc <= 49152 and nc % 2 == 0) > 50
    wide, wrecs = sa.oracle_run(mr.even_room(wide=True), SEED)      # (the lone point at the origin: a region of its own, no step)
    assert sorted(r['nc'] for r in wrecs.values()) == ncs
    assert [(r['steps'], r['points'], r['reason']) for r in wide.regions] == [(256, 49664, 'noexpand'), (2, 3, 'noneighbor'), (0, 1, 'noneighbor')]


def test_wide_and_cut_rooms_grow_alike(classes):
    _, want, _ = classes
    for room in (mr.classes_room(wide=True), mr.cut_room(), mr.classes_room(F=12)):
        got, recs = sa.oracle_run(room, SEED)
        k = len(room['strips'])
        key = lambda r: (r['steps'], r['points'], r['reason'])
        assert [key(r) for r in got.regions[:k]] == [key(r) for r in want.regions[:k]]
        assert max(r['ne'] for r in recs.values()) <= 512


def test_every_boundary_and_both_parities(classes, big, even):
    ncs = [r['nc'] for _, _, recs in (classes, big, even) for r in recs.values()]
    for size in (256, 257, 1024, 1025, 4096, 4097, 16384, 16385, 49152, 49153):
        assert size in ncs
    for k, (lo, hi) in enumerate(mr.SIZE_CLASSES):
        par = {nc & 1 for nc in ncs if lo <= nc <= hi}
        assert par == {0, 1}, (lo, hi, par)      # (above 49152: the big room's 49153 and the even room's 49276 / 49470 / 49664)


def test_sampled_selection_takes_both_paths(classes, big):
    """16385 .. 49152 points: lrg_median_block_sampled selects inside its bracket (at most 8192 keys there, both middle ranks
    inside) or falls back to the full bisection.  Both occur, and a bracket above 8192 keys occurs, over (record, channel)."""
    lo, hi = mr.SIZE_CLASSES[4]
    inside_counts, bracket_path = [], []
    for room, _, recs in (classes, big):
        pts = room['points']
        hits = [r for r in recs.values() if lo <= r['nc'] <= hi]
        assert hits
        for r in hits[::8] + hits[-1:]:
            cur = np.flatnonzero(sa.mask_of(r))
            for ch in (0, 1, 6, 7, 8, 9, 10, 11, 12):
                _, inside, ok = mr.sampled_bracket(pts[cur, ch], r['nc'])
                inside_counts.append(inside)
                bracket_path.append(ok)
    assert max(inside_counts) > 8192 and min(inside_counts) < 8192
    assert any(bracket_path) and not all(bracket_path)


# ---------------------------------------------------------------------------------------------------------------------------
# planted faults
# ---------------------------------------------------------------------------------------------------------------------------
def _ulp(x):
    return np.nextafter(np.float32(x), np.float32(np.inf))


def plant_centre_ulp(st, exp, room):
    st['center'][6] = _ulp(st['center'][6])


def plant_upper_middle(st, exp, room):
    nc = exp['slot']['nc']
    assert nc % 2 == 0
    v = np.sort(room['points'][exp['cur_list'], 6])
    assert v[nc // 2] != v[nc // 2 - 1]
    st['center'][6] = v[nc // 2]


def plant_swapped_list(st, exp, room):
    st['cur_list'][[3, 4]] = st['cur_list'][[4, 3]]


def plant_swapped_candidates(st, exp, room):
    st['cand_list'][[0, 1]] = st['cand_list'][[1, 0]]


def plant_sample_position(st, exp, room):
    j = len(st['sample_in']) - 1
    st['sample_in'][j] = (st['sample_in'][j] + 1) % exp['slot']['nc']


def plant_row_centred_twice(st, exp, room):
    F = st['x_in'].shape[1]
    st['x_in'][2] = exp['x_in_centred'][2] - exp['center'][:F]


def plant_row_centred_once_where_raw(st, exp, room):
    st['x_nb'][1] = exp['x_nb_centred'][1]


def plant_flag(st, exp, room):
    st['upd_nb'][0, 3] = 1.0 - st['upd_nb'][0, 3]


def plant_mask_bit(st, exp, room):
    st['mask'][np.flatnonzero(~st['mask'])[0]] = True


def plant_box(st, exp, room):
    st['slot']['mx'][1] += 1


def plant_logit(st, exp, room):
    st['add_logits'][0, 1] = _ulp(st['add_logits'][0, 1])


def plant_set_row(st, exp, room):
    st['inlier'][-1, 0] = _ulp(st['inlier'][-1, 0])


def plant_set_flag(st, exp, room):
    st['gt_add'][-1] ^= 1


FAULTS = [('general', plant_centre_ulp), ('greedy', plant_centre_ulp), ('step', plant_centre_ulp),
          ('general', plant_upper_middle), ('greedy', plant_upper_middle), ('free', plant_upper_middle),
          ('general', plant_swapped_list), ('greedy', plant_swapped_list), ('free', plant_swapped_candidates), ('step', plant_swapped_list),
          ('general', plant_sample_position), ('step', plant_sample_position),
          ('general', plant_row_centred_twice), ('greedy', plant_row_centred_once_where_raw), ('free', plant_row_centred_once_where_raw),
          ('greedy', plant_flag), ('general', plant_flag), ('greedy', plant_mask_bit), ('free', plant_box), ('general', plant_logit),
          ('step', plant_set_row), ('step', plant_set_flag)]


@pytest.fixture(scope='module')
def a_step(classes):
    """An even count inside the (32, 1024) strip: 18 x 18 points, 37 candidates -- both sets padded."""
    room, _, recs = classes
    first = room['strips'][2][0]
    rec = recs[(first, 0, 17)]
    assert rec['nc'] == 324 and rec['ne'] == 37
    return room, rec, sa.expected(room, rec)


def test_the_comparer_accepts_the_oracle_itself(a_step, classes):
    room, rec, exp = a_step
    for form in sa.FORMS:
        sa.compare(sa.perfect_state(exp, form, logits=True), exp, form, logits=form != 'step')
    # ... at a full inlier set too (a prefix of the permutation)
    _, _, recs = classes
    full = recs[(room['strips'][3][0], 0, 32)]
    assert full['nc'] == 1025
    exp = sa.expected(room, full)
    for form in sa.FORMS:
        sa.compare(sa.perfect_state(exp, form), exp, form)


@pytest.mark.parametrize('form,plant', FAULTS, ids=['%s-%s' % (f, p.__name__[6:]) for f, p in FAULTS])
def test_the_comparer_fails_on_a_planted_fault(a_step, form, plant):
    room, rec, exp = a_step
    st = sa.perfect_state(exp, form, logits=True)
    plant(st, exp, room)
    with pytest.raises(AssertionError, match='oracle'):
        sa.compare(st, exp, form, 'planted', logits=form != 'step')


def test_the_comparer_insists_on_what_a_form_leaves_behind(a_step):
    room, rec, exp = a_step
    st = sa.perfect_state(exp, 'general')
    del st['sample_in']
    with pytest.raises(AssertionError, match='left no'):
        sa.compare(st, exp, 'general')
    with pytest.raises(AssertionError, match='left no'):
        sa.compare(sa.perfect_state(exp, 'greedy'), exp, 'greedy', logits=True)
