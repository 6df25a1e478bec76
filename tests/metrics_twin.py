"""A NumPy float64 restatement of the device's evaluation pass (csrc/lrg_metrics.hip), for the tests of metrics_gpu: the contingency
table, the integer sums, the entropies and the mutual information term by term, the expected mutual information from one table
T[k] = gammaln(k + 1) with per-pair partial sums, the greedy matching in the prepared visit order, and metrics_gpu's host finish.
Also the labelings the tests share (``cases``)."""
import glob
import os

import numpy as np
from scipy.special import gammaln

from learn_region_grow_amd import metrics_gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
EPS = float(np.finfo('float64').eps)
LDS_CELLS = 8192          # csrc/lrg_metrics.hip MT_LDS_CELLS: tables up to this many cells are counted in LDS, larger ones with global atomics


def twin_sums(gt_row, n_gt, cluster_label, n_cluster):
    """(int_sums[6], float_sums[4], cont) as lrg_metrics_batch makes them."""
    cont = np.zeros((n_gt, n_cluster + 1), dtype=np.int64)
    np.add.at(cont, (gt_row, cluster_label), 1)
    a, b = cont.sum(axis=1), cont.sum(axis=0)
    N = int(a.sum())
    ints = [int((cont * cont).sum()), int((a * a).sum()), int((b * b).sum()), N, int((a > 0).sum()), int((b > 0).sum())]
    logN = np.log(float(N))

    def entropy(p):
        p = p[p > 0].astype(np.float64)
        return -float(np.sum((p / N) * (np.log(p) - logN)))
    gi, ji = np.nonzero(cont)
    v = cont[gi, ji].astype(np.float64)
    nm = v / N
    log_outer = -np.log((a[gi] * b[ji]).astype(np.float64)) + logN + logN
    mi = nm * (np.log(v) - logN) + nm * log_outer
    mi = float(np.where(np.abs(mi) < EPS, 0.0, mi).sum())
    T = gammaln(np.arange(N + 1) + 1.0)
    emi = 0.0
    for i in np.nonzero(a)[0]:
        ai = int(a[i])
        for j in np.nonzero(b)[0]:
            bj = int(b[j])
            nij = np.arange(max(1, ai + bj - N), min(ai, bj) + 1)
            gln = T[ai] + T[bj] + T[N - ai] + T[N - bj] - (T[nij] + T[N]) - T[ai - nij] - T[bj - nij] - T[N - ai - bj + nij]
            term = (nij / float(N)) * ((logN + np.log(nij.astype(np.float64))) - np.log(float(ai)) - np.log(float(bj))) * np.exp(gln)
            emi += float(term.sum())                 # (a partial per pair)
    return ints, [entropy(a), entropy(b), mi, emi], cont


def twin_room_metrics(obj_id, cluster_label, order='size', with_scores=True):
    """metrics.room_metrics (order='size') / room_metrics_set_order (order='set') the way the device pass computes them."""
    cluster_label = np.asarray(cluster_label)
    prep = metrics_gpu.prepare_ground_truth(obj_id, order)
    C, G = int(cluster_label.max()), prep['n_gt']
    cont = np.zeros((G, C + 1), dtype=np.int64)
    np.add.at(cont, (prep['gt_row'], cluster_label), 1)
    a, b = cont.sum(axis=1), cont.sum(axis=0)
    dt = np.zeros(C, dtype=np.uint8)
    cmap = np.zeros(C + 1, dtype=np.int64)
    best, gt_match = np.zeros(G), 0
    for k in range(G):
        g = prep['order'][k]
        free = np.nonzero(dt == 0)[0] + 1
        if len(free) == 0:
            continue
        inter = cont[g, free]
        iou = 1.0 * inter / (a[g] + b[free] - inter)
        best[k] = iou.max()
        hit = np.nonzero(iou > 0.5)[0]
        if len(hit):
            j = free[hit[0]]
            dt[j - 1] = 1
            cmap[j] = prep['relabel'][k]
            gt_match += 1
    for j in range(1, C + 1):
        if not dt[j - 1]:
            cmap[j] = j + prep['unmatched_base']
    ints = floats = None
    if with_scores:
        ints, floats, _ = twin_sums(prep['gt_row'], G, cluster_label, C)
    return metrics_gpu.finish_room(C, G, dt, gt_match, best, cmap[cluster_label], ints, floats)


def golden_rooms():
    out = []
    for f in sorted(glob.glob(os.path.join(GOLDEN, '*room*.npz'))):
        z = np.load(f)
        if 'obj_id' in z.files and 'filled_label' in z.files:
            out.append((os.path.basename(f)[:-4], z['obj_id'], z['filled_label']))
    assert len(out) == 6
    return out


def cases():
    """(name, obj_id, cluster_label): the smallest labelings at which each piece of the pass can go wrong."""
    rng = np.random.RandomState(7)
    out = [('one_class_one_cluster', np.full(100, 3), np.ones(100, dtype=np.int64)),
           ('one_class_four_clusters', np.full(130, 5), 1 + np.arange(130) % 4),
           ('four_classes_one_cluster', np.arange(130) % 4, np.ones(130, dtype=np.int64)),
           ('perfect_7', np.arange(257) % 7 + 2, np.arange(257) % 7 + 1)]
    # a + b > N: the lower bound a + b - N of the nij range is live
    out.append(('lower_bound_live', np.repeat([1, 2], [700, 301]), np.repeat([1, 2], [650, 351])))
    obj = rng.choice([-7, -2, 3, 40, 41, 1000], size=1000)
    lab = rng.choice([0, 2, 5, 9], size=1000)
    lab[obj == 40] = 5
    out.append(('gapped_negative_ids', obj, lab))
    # 3 x 5001 = 15 003 cells: past the LDS budget of 8192 cells, global atomics
    lab = rng.permutation(np.concatenate([np.arange(1, 5001), rng.randint(1, 5001, size=1000)]))
    out.append(('3x5000_global_table', rng.randint(0, 3, size=6000), lab))
    # 64 x 128 = 8192 cells: the largest table counted in LDS; 64 x 129: the first past it (80 % agreement, as the case below)
    for c in (127, 128):
        obj = rng.randint(0, 64, size=3000)
        lab = np.where(rng.rand(3000) < 0.8, obj + 1, rng.randint(1, c + 1, size=3000))
        lab[:c] = np.arange(1, c + 1)
        out.append(('64x%d_lds_edge' % c, obj, lab))
    obj = rng.randint(0, 20, size=4097)
    lab = np.where(rng.rand(4097) < 0.8, obj + 1, rng.randint(1, 31, size=4097))
    lab[:30] = np.arange(1, 31)
    out.append(('20x30_agree80', obj, lab))
    out.append(('n1', np.array([4]), np.array([1])))
    out.append(('n2_split', np.array([4, 9]), np.array([1, 2])))
    return out + golden_rooms()
