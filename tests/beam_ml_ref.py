"""Test twin: the beam search of one room with ``scoring='np' | 'ml'``, an error bound on every 'ml' score, and a mode that
FOLLOWS a device run level by level (test infrastructure; not collected by pytest).

It is oracle/beam_ref.py (the project's restatement of test_beam_search.py:143-290, pinned to the reference script's output)
restated with the score the reference computes per child under ``--scoring ml`` (:237-257, :273):

  * every one of the NUM_NEIGHBOR_POINT neighbour rows, padded copies included, is un-centred and re-voxelised; a row whose voxel
    lies in the set of voxels whose draw fired contributes log(conf_i) / NUM_NEIGHBOR_POINT, any other row
    log(1 - conf_i) / NUM_NEIGHBOR_POINT (membership is by voxel: a copy of a fired point counts as fired whatever its own draw said);
  * the remove side likewise over the inlier rows with rmv_conf -- also divided by NUM_NEIGHBOR_POINT, the script's quirk, kept;
  * newScore = (currentScore + addLogProb) + rmvLogProb; the seed-only head has score 0;
  * Q = sorted(newQ, key=score, reverse=True)[:BEAM_WIDTH], a stable sort, and only then are emptied masks dropped
    (oracle/beam_ref.py:139-140), so an emptied mask with a high score leaves the queue shorter.

Arithmetic as the project fixed it for the restart score (oracle/grow_ref.py:161-170): float32 confidences, float32 log, float32
division, the terms of a side summed in float64.  log(0) = -inf is a legal score: it orders last, ties among -inf keep child order.

The bound.  Children of one parent share most rows, so candidate scores are often equal or a few ulps apart, and the device's
expf / logf differ from NumPy's by ulps: a device run may order such a pair the other way and both are right.  Beside every score the
twin therefore keeps E, a bound on |device score - twin score| for the SAME logits, masks and rows.  Its constants (in units of
2**-23 relative, one float32 ulp at most):

  CONF_ULP = 8    conf = e1 / (e0 + e1) with e = exp(logit - max): one of the two exponentials is exp(0) = 1 exactly, the other is off
                  by <= 1 ulp on the device (HIP math API: expf, maximum error 1 ulp) and <= 2.52 ulp in NumPy (its float32 SIMD exp,
                  "max ULP error 2.52", NumPy 1.17 release notes) -- 3.52 between the two; the correctly rounded add and divide give
                  half an ulp each on each side, 2 more: 5.52, taken as 8 (the relative error of conf never exceeds that of the inexact
                  exponential, in the numerator or in the denominator).
  SUB_ULP  = 1    1 - conf: the correctly rounded subtraction, half an ulp on each side.
  LOG_ULP  = 5    logf on the device <= 1 ulp (HIP math API), NumPy's float32 SIMD log <= 3.83 ulp (same release notes): 4.83.
  DIV_ULP  = 1    the correctly rounded division by NUM_NEIGHBOR_POINT, half an ulp on each side.

and they propagate as  |d log x| <= -log(1 - dx / x)  with dx = CONF_ULP ulp of conf (+ SUB_ULP ulp of x where x = 1 - conf), plus
LOG_ULP + DIV_ULP ulp of the term itself; infinite where dx >= x or x is subnormal.  x = 0 exactly (a logit difference beyond -104:
exp underflows to 0 in every float32 exp) gives the term -inf with no error.  The float64 sums add N * 2**-52 relative.  E accumulates
along the path from the seed.  With saturated confidences (trained weights) dx / x approaches 1 and the bound explodes: the parity
tests use the synthetic weights and rooms with furniture, where it stays near 1e-5 relative.

Follow mode (``follow=`` a device trace, {(seed, level): [(child ordinal, mask size, score), ...]} or the list form of
BeamSearchGrower(trace=True)): at every level the twin computes its own candidates, reads the device's record, checks it --
every entry an updated child, its size the twin's, its score within E, every two consecutive entries in an order the twin's scores
cannot refute (twin[a] - twin[b] >= -(E_a + E_b)), every updated child left out losing to the last entry by the same test, fewer than
beam_width entries only if every updated child is listed -- and continues from the DEVICE's queue, the emptied masks dropped.  It counts
the pairs compared and the undecided ones (gap within E_a + E_b).  A record it can refute raises FollowError.
"""
import numpy as np

from oracle import lrgnet_ref
from oracle.grow_ref import GrowResult, fill_unlabeled, pack_voxels, voxelize
from oracle.rng_ref import PURPOSE_ADD, PURPOSE_INLIER, PURPOSE_NEIGHBOR, PURPOSE_RMV

CONF_ULP, SUB_ULP, LOG_ULP, DIV_ULP = 8.0, 1.0, 5.0, 1.0
EPS32 = 2.0 ** -23
EPS64 = 2.0 ** -52
TINY32 = 2.0 ** -126


class FollowError(AssertionError):
    pass


def small_room(seed, n_raw, furniture=0, room_id=0):
    """The rooms of tests/test_gpu_beam.py: a synthetic room, preprocessed on the host"""
    from learn_region_grow_amd import preprocess, synthetic
    raw = (synthetic.area5_shaped_room(n_raw, seed, n_furniture=furniture) if furniture
           else synthetic.generate_room_points(n_raw, seed)).astype(np.float32)
    p = preprocess.preprocess_room(raw[:, :6], raw[:, 6].astype(int), raw[:, 7].astype(int))
    return dict(points=p['points'], obj_id=p['obj_id'], order=p['order'], room_id=room_id)


def side_terms(rows, conf, mask, center, resolution, num_neighbor):
    """One side of a child's score.  rows [N, F] float32 (centred), conf [N] float32, mask [N] bool (the draws that fired),
    center [F].  -> (term [N] float32, err [N] float64, in_set [N] bool): term_i = log(conf_i or 1 - conf_i) / num_neighbor as
    float32, err_i the bound on |device term - term_i|."""
    q = np.array(rows, dtype=np.float32)
    q[:, :2] += np.asarray(center, dtype=np.float32)[:2]                          # :240 / :252 (row by row upstream; same float32 adds)
    keys = pack_voxels(voxelize(q[:, :3], resolution))
    mask = np.asarray(mask, dtype=bool)
    in_set = np.isin(keys, keys[mask]) if mask.any() else np.zeros(len(keys), bool)
    c32 = np.asarray(conf, dtype=np.float32)
    x = np.where(in_set, c32, np.float32(1.0) - c32).astype(np.float32)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        lg = np.log(x)                                                            # float32
        term = (lg / np.float32(num_neighbor)).astype(np.float32)                 # :243-245 / :255-257 (both / NUM_NEIGHBOR_POINT)
        x64, c64 = x.astype(np.float64), c32.astype(np.float64)
        dx = CONF_ULP * EPS32 * c64 + np.where(in_set, 0.0, SUB_ULP * EPS32 * x64)
        ratio = np.where(x64 > 0, dx / np.where(x64 > 0, x64, 1.0), 0.0)
        dlog = np.where(ratio < 1.0, -np.log1p(-np.minimum(ratio, 1.0 - 2.0 ** -50)), np.inf)      # |log(x -+ dx) - log x|
        err = (dlog + (LOG_ULP + DIV_ULP) * EPS32 * np.abs(lg.astype(np.float64))) / float(num_neighbor)
        err = np.where(x64 == 0, 0.0, np.where(x64 < TINY32, np.inf, err))        # exact 0: -inf on both sides; subnormal: no ulp bound
    return term, err, in_set


def side_sum(term, err):
    """(float64 sum of the float32 terms, bound on it)"""
    t64 = term.astype(np.float64)
    with np.errstate(invalid='ignore'):
        s = float(np.sum(t64))
    finite = np.isfinite(t64)
    e = float(np.sum(err)) + len(t64) * EPS64 * float(np.sum(np.abs(t64[finite])))
    return s, e


def child_sides(neighbor, inlier, add_conf, rmv_conf, add_mask, rmv_mask, center, resolution, num_neighbor):
    """-> dict(add, add_err, rmv, rmv_err, add_terms, rmv_terms, add_term_err, rmv_term_err): both sides of one child"""
    ta, ea, _ = side_terms(neighbor, add_conf, add_mask, center, resolution, num_neighbor)
    tr, er, _ = side_terms(inlier, rmv_conf, rmv_mask, center, resolution, num_neighbor)
    a, aerr = side_sum(ta, ea)
    r, rerr = side_sum(tr, er)
    return dict(add=a, add_err=aerr, rmv=r, rmv_err=rerr, add_terms=ta, rmv_terms=tr, add_term_err=ea, rmv_term_err=er)


def child_score(parent_score, parent_err, sides):
    """newScore = (currentScore + addLogProb) + rmvLogProb (:273) and its bound"""
    s = (parent_score + sides['add']) + sides['rmv']
    e = parent_err + sides['add_err'] + sides['rmv_err']
    if np.isfinite(s):
        e += 4 * EPS64 * (abs(parent_score) + abs(sides['add']) + abs(sides['rmv']))
    return s, e


def not_refuted(sa, sb, bound):
    """May `a` stand before `b` in a descending order, as far as the twin's scores sa, sb and the bound can tell?"""
    if sa == sb:                      # (also -inf, -inf)
        return True
    if sa == -np.inf:
        return False
    if sb == -np.inf:
        return True
    return sa - sb >= -bound


def undecided(sa, sb, bound):
    if sa == sb:
        return True
    if not (np.isfinite(sa) and np.isfinite(sb)):
        return False
    return abs(sa - sb) <= bound


def trace_dict(trace):
    """BeamSearchGrower's list form [(seed, level, entries), ...] -> {(seed, level): entries}"""
    if isinstance(trace, dict):
        return trace
    out = {}
    for seed, level, entries in trace:
        assert (seed, level) not in out, 'two records for seed %d level %d' % (seed, level)
        out[(int(seed), int(level))] = list(entries)
    return out


def beam_room(points, obj_id, order, weights, stream, *, room_id=0, resolution=0.1, lite=0, num_inlier=512, num_neighbor=512,
              cluster_threshold=10, beam_width=3, search_width=3, policy='net', net_fn=None, fill=True, scoring='np', follow=None):
    """oracle.beam_ref.beam_room with scoring= and follow=.  The result also carries beam_trace (the list form, with the twin's own
    choices -- or, following, the device's), beam_trace_err (per record, the bounds of its entries), pairs_compared, pairs_undecided
    and worst_rel_bound (max E / |score| over the finite scores seen)."""
    if scoring not in ('np', 'ml'):
        raise ValueError(scoring)
    ml = scoring == 'ml'
    follow = trace_dict(follow) if follow is not None else None
    points = np.ascontiguousarray(points, dtype=np.float32)
    obj_id = np.asarray(obj_id)
    N, F = points.shape
    res = GrowResult()
    res.beam_trace, res.beam_trace_err = [], []
    res.pairs_compared = res.pairs_undecided = 0
    res.worst_rel_bound = 0.0
    if net_fn is None:
        def net_fn(xi, xn):
            return lrgnet_ref.forward(weights, xi, xn, lite=lite)
    point_voxels = voxelize(points[:, :3], resolution)            # :143
    room_keys = pack_voxels(point_voxels)
    cluster_label = np.zeros(N, dtype=np.int64)
    cluster_id = 1
    visited = np.zeros(N, dtype=bool)
    inlier_points = np.zeros((1, num_inlier, F), dtype=np.float32)
    neighbor_points = np.zeros((1, num_neighbor, F), dtype=np.float32)
    add_acc = rmv_acc = float('nan')
    used = set()

    for seed_id in np.arange(N)[np.asarray(order)]:               # :154
        if visited[seed_id]:
            continue
        seed_voxel = point_voxels[seed_id]
        target_id = obj_id[seed_id]
        gt_mask = obj_id == target_id
        currentMask = np.zeros(N, dtype=bool)                     # :164-165
        currentMask[seed_id] = True
        seqMinDims, seqMaxDims = seed_voxel.copy(), seed_voxel.copy()
        steps = 0
        stuck = 0
        bestMask = currentMask
        Q = [dict(score=0.0, err=0.0, mask=currentMask)]          # :164, :174: the seed-only head, score 0
        level = 0
        stalled = False
        while len(Q) > 0 and not stalled:                         # :179
            newQ = []
            for qid, entry in enumerate(Q):
                currentMask = entry['mask']
                minDims = point_voxels[currentMask, :].min(axis=0)    # :186-187
                maxDims = point_voxels[currentMask, :].max(axis=0)
                if qid == 0:                                          # :188-198
                    bestMask = currentMask
                    if not np.any(minDims < seqMinDims) and not np.any(maxDims > seqMaxDims):
                        if stuck >= 1:
                            stalled = True
                            break
                        stuck += 1
                    else:
                        stuck = 0
                    seqMinDims = np.minimum(seqMinDims, minDims)
                    seqMaxDims = np.maximum(seqMaxDims, maxDims)
                currentPoints = points[currentMask, :]
                mask = np.logical_and(np.all(point_voxels >= minDims - 1, axis=1), np.all(point_voxels <= maxDims + 1, axis=1))   # :203-207
                mask = np.logical_and(mask, np.logical_not(currentMask))
                mask = np.logical_and(mask, np.logical_not(visited))
                expandPoints = points[mask, :]
                expandClass = obj_id[mask] == target_id
                rejectClass = obj_id[currentMask] != target_id
                if len(expandPoints) == 0:                            # :212
                    continue
                for search_id in range(search_width):
                    ordinal = qid * search_width + search_id
                    ctx = (int(seed_id), ordinal, level)
                    nc, ne = len(currentPoints), len(expandPoints)
                    subset = stream.sample(nc, num_inlier, PURPOSE_INLIER, ctx)          # :216-219
                    center = np.median(currentPoints, axis=0)                             # :220
                    ep = np.array(expandPoints)                                            # :221-223
                    ep[:, :2] -= center[:2]
                    ep[:, 6:] -= center[6:]
                    inlier_points[0, :, :] = np.array(currentPoints[subset, :])            # :224-226
                    inlier_points[0, :, :2] -= center[:2]
                    inlier_points[0, :, 6:] -= center[6:]
                    input_remove = np.asarray(rejectClass)[subset].astype(np.int32)        # :227
                    subset_n = stream.sample(ne, num_neighbor, PURPOSE_NEIGHBOR, ctx)      # :228-231
                    neighbor_points[0, :, :] = ep[subset_n, :]                             # :232
                    input_add = np.asarray(expandClass)[subset_n].astype(np.int32)         # :233
                    add, rmv = net_fn(inlier_points, neighbor_points)                      # :234-235
                    add = np.asarray(add, dtype=np.float32)
                    rmv = np.asarray(rmv, dtype=np.float32)
                    _, add_acc, rmv_acc = lrgnet_ref.logged_scalars(add, rmv, input_add[None], input_remove[None])
                    res.total_steps += 1
                    add_conf = lrgnet_ref.confidence(add[0])                               # :237-238
                    rmv_conf = lrgnet_ref.confidence(rmv[0])
                    u_add = stream.uniform(len(add_conf), PURPOSE_ADD, ctx)                # :239-240
                    u_rmv = stream.uniform(len(rmv_conf), PURPOSE_RMV, ctx)
                    if policy == 'net':
                        add_mask = u_add < add_conf
                        rmv_mask = u_rmv < rmv_conf
                        for u_, c_ in ((u_add, add_conf), (u_rmv, rmv_conf)):
                            d_ = np.abs(np.asarray(u_, np.float64) - c_)
                            res.min_margin = min(res.min_margin, float(d_.min()))
                            res.min_rel_margin = min(res.min_rel_margin, float((d_ / (c_ * (1.0 - c_) + 1e-6)).min()))
                    elif policy == 'gt':
                        add_mask = input_add.astype(bool)
                        rmv_mask = input_remove.astype(bool)
                    else:
                        raise ValueError(policy)
                    score, err = 0.0, 0.0
                    if ml:                                                                  # :237-257, before the rows are consumed
                        score, err = child_score(entry['score'], entry['err'],
                                                 child_sides(neighbor_points[0], inlier_points[0], add_conf, rmv_conf, add_mask, rmv_mask,
                                                             center, resolution, num_neighbor))
                    addPoints = neighbor_points[0, :, :][add_mask]                          # :241-243
                    addPoints[:, :2] += center[:2]
                    addVoxels = voxelize(addPoints[:, :3], resolution)
                    rmvPoints = inlier_points[0, :, :][rmv_mask]                            # :252-254
                    rmvPoints[:, :2] += center[:2]
                    rmvVoxels = voxelize(rmvPoints[:, :3], resolution)
                    in_add = np.isin(room_keys, pack_voxels(addVoxels)) if len(addVoxels) else np.zeros(N, bool)
                    in_rmv = np.isin(room_keys, pack_voxels(rmvVoxels)) if len(rmvVoxels) else np.zeros(N, bool)
                    newMask = currentMask.copy()                                            # :264-270
                    updated = bool(np.any(in_add & ~newMask))
                    newMask |= in_add
                    newMask[in_rmv] = False
                    steps += 1                                                              # :274
                    if updated:                                                             # :275-280
                        size = int(np.sum(newMask))
                        newQ.append(dict(score=score if ml else size, err=err, mask=newMask, size=size, ordinal=ordinal))
            if stalled:
                break
            # ---- :282: the best beam_width by score (stable), THEN without the emptied masks ----
            for e in newQ:
                if ml and np.isfinite(e['score']) and e['score'] != 0:
                    res.worst_rel_bound = max(res.worst_rel_bound, e['err'] / abs(e['score']))
            if follow is None:
                best = sorted(newQ, key=lambda e: e['score'], reverse=True)[:beam_width]
            else:
                try:
                    best = _check_record(follow, used, int(seed_id), level, newQ, beam_width, ml, res)
                except FollowError as e:
                    e.result = res          # (so far: a caller may want min_rel_margin, the closest draw on the way here)
                    raise
            res.beam_trace.append((int(seed_id), level, [(e['ordinal'], e['size'], float(e['score'])) for e in best]))
            res.beam_trace_err.append([e['err'] for e in best])
            Q = [e for e in best if e['size'] > 0]    # an emptied mask has no bounding box (:186 would raise); dropped here
            level += 1
        visited[bestMask] = True                                  # :289
        labeled = bool(np.sum(bestMask) > cluster_threshold)
        rec = dict(seed=int(seed_id), target=int(target_id), steps=int(steps), points=int(np.sum(bestMask)),
                   gt=int(np.sum(gt_mask)),
                   iou=float(1.0 * np.sum(np.logical_and(gt_mask, bestMask)) / np.sum(np.logical_or(gt_mask, bestMask))),
                   add_acc=float(add_acc), rmv_acc=float(rmv_acc), labeled=labeled)
        if labeled:                                               # :290-293
            cluster_label[bestMask] = cluster_id
            cluster_id += 1
        res.regions.append(rec)
    if follow is not None and len(used) != len(follow):
        e = FollowError('the device trace holds %d records the search never reached: %s' % (
            len(follow) - len(used), sorted(set(follow) - used)[:5]))
        e.result = res
        raise e
    res.cluster_label = cluster_label
    res.filled_label = fill_unlabeled(points, cluster_label) if fill else None
    return res


def _check_record(follow, used, seed, level, newQ, beam_width, ml, res):
    """The device's record of (seed, level) against the twin's candidates newQ (child order): -> the device's best list as the twin's
    entries.  Raises FollowError on anything the twin's scores and bounds can refute."""
    where = 'seed %d level %d' % (seed, level)
    if (seed, level) not in follow:
        raise FollowError('%s: no device record' % where)
    used.add((seed, level))
    record = follow[(seed, level)]
    by_ord = {e['ordinal']: e for e in newQ}
    if len(record) > beam_width:
        raise FollowError('%s: %d entries for a beam of %d' % (where, len(record), beam_width))
    if len(set(o for o, _, _ in record)) != len(record):
        raise FollowError('%s: a child is listed twice: %s' % (where, record))
    best = []
    for o, size, score in record:
        if o not in by_ord:
            raise FollowError('%s: child %d is listed but its mask did not change (updated children: %s)' % (where, o, sorted(by_ord)))
        e = by_ord[o]
        if size != e['size']:
            raise FollowError('%s child %d: device mask of %d points, twin %d' % (where, o, size, e['size']))
        if ml:
            ok = score == e['score'] or (np.isfinite(score) and np.isfinite(e['score']) and abs(score - e['score']) <= e['err'])
        else:
            ok = score == float(size)
        if not ok:
            raise FollowError('%s child %d: device score %r, twin %r, bound %.3g' % (where, o, score, e['score'], e['err']))
        best.append(e)
    if len(best) < beam_width and len(best) != len(newQ):
        raise FollowError('%s: %d entries listed, beam %d, but %d children were updated' % (where, len(best), beam_width, len(newQ)))

    def pair(a, b, what):
        bound = a['err'] + b['err']
        res.pairs_compared += 1
        if not not_refuted(a['score'], b['score'], bound):
            raise FollowError('%s: %s: child %d (twin score %r) stands before child %d (%r), bound %.3g' % (
                where, what, a['ordinal'], a['score'], b['ordinal'], b['score'], bound))
        if undecided(a['score'], b['score'], bound):
            res.pairs_undecided += 1
            # an exact tie keeps child order (a stable sort) wherever the device's own scores tie too
    for a, b in zip(best[:-1], best[1:]):
        pair(a, b, 'consecutive entries')
    listed = set(e['ordinal'] for e in best)
    if best:
        for e in newQ:
            if e['ordinal'] not in listed:
                pair(best[-1], e, 'left out')
    return best
