"""Twin of the device batch assembly (csrc/lrg_assemble.hip, train_data.TupleStore.assemble), for tests/test_assemble_host.py and
tests/test_gpu_assemble.py: NumPy and oracle.rng_ref only.

The job is the reference's train_region_grow.py:156-175 -- every tuple of a batch padded / subsampled to k points a side -- under the
counter stream: slot j of tuple t with N rows takes row ``CounterStream(rng_seed, t).sample(N, k, purpose, (0, pass, epoch))[j]``.
"""
import numpy as np

from oracle import rng_ref

TRAIN_INLIER, TRAIN_NEIGHBOR = 11, 12            # csrc/lrg_rng.h: LRG_PURPOSE_TRAIN_INLIER / _NEIGHBOR
PASS_TRAIN, PASS_VALIDATION = 0, 1


def positions(rng_seed, t, N, k, purpose, epoch, pass_):
    """The k row positions (< N) of tuple t's side of N rows."""
    return np.asarray(rng_ref.CounterStream(rng_seed, t).sample(int(N), int(k), purpose, (0, int(pass_), int(epoch))), dtype=np.int64)


def assemble_side(rows, labels, row_start, row_count, order, k, F, rng_seed, epoch, pass_, purpose):
    """rows [*, S] float32, labels [*] int32, row_start / row_count per tuple, order [B] tuple ids
    -> out_rows [B,k,F] float32, out_labels [B,k] int32, positives [B] int32."""
    B = len(order)
    out_rows = np.zeros((B, k, F), dtype=np.float32)
    out_labels = np.zeros((B, k), dtype=np.int32)
    for b, t in enumerate(order):
        at = int(row_start[t]) + positions(rng_seed, int(t), row_count[t], k, purpose, epoch, pass_)
        out_rows[b] = rows[at, :F]
        out_labels[b] = labels[at]
    return out_rows, out_labels, out_labels.sum(axis=1).astype(np.int32)


def assemble_batch(tuples, order, k_in, k_nb, F, rng_seed, epoch, pass_):
    """tuples: dict of the four flat host arrays points / remove / neighbor_points / add and the tables start_in / count_in / start_nb /
    count_nb -> (inlier [B,k_in,F], neighbor [B,k_nb,F], add [B,k_nb], remove [B,k_in], positives_remove [B], positives_add [B]), the
    first four in stage.assemble_batch's order."""
    xi, ir, pr = assemble_side(tuples['points'], tuples['remove'], tuples['start_in'], tuples['count_in'], order, k_in, F, rng_seed, epoch, pass_,
                               TRAIN_INLIER)
    xn, ia, pa = assemble_side(tuples['neighbor_points'], tuples['add'], tuples['start_nb'], tuples['count_nb'], order, k_nb, F, rng_seed, epoch,
                               pass_, TRAIN_NEIGHBOR)
    return xi, xn, ia, ir, pr, pa


def constructed_tuples(stride=13, seed=0):
    """Eight tuples whose sides have [1, 2, 63, 64, 65, 129, 1024, 3000] and [3000, 1024, 129, 65, 64, 63, 2, 1] rows: every element of the
    rows unique (arange-derived), random 0/1 flags with tuple 2 all 0 and tuple 5 all 1 on both sides, and a gap of rows that no tuple owns
    after tuple 3 (as a tuple left out of the tables leaves one)."""
    cin = np.array([1, 2, 63, 64, 65, 129, 1024, 3000], dtype=np.int32)
    cnb = cin[::-1].copy()
    rs = np.random.RandomState(seed)
    out = {}
    for side, cnt, rows_key, lab_key, base in (('in', cin, 'points', 'remove', 0.0), ('nb', cnb, 'neighbor_points', 'add', 0.5)):
        gap = np.where(np.arange(8) == 3, 37, 0)
        start = np.concatenate([[5], 5 + np.cumsum(cnt + gap)[:-1]]).astype(np.int64)
        total = int(start[-1] + cnt[-1] + 11)
        rows = (np.arange(total * stride, dtype=np.float64) + base).astype(np.float32).reshape(total, stride)      # below 2^24: exact and unique
        lab = rs.randint(0, 2, total).astype(np.int32)
        lab[start[2]:start[2] + cnt[2]] = 0
        lab[start[5]:start[5] + cnt[5]] = 1
        out[rows_key], out[lab_key], out['start_' + side], out['count_' + side] = rows, lab, start, cnt
    return out
