"""CPU: the restatement the GPU tests of the MCPNet trainer lean on (tests/mcpnet_train_ref.py), checked on its own, and the host
side of learn_region_grow_amd.mcpnet_train: the checkpoint layout, even_sampling and the two metrics.

tests/golden/mcpnet_model5_names.json holds [name, shape, dtype] of the 27 entries of the reference's shipped
models/mcpnet_model5.ckpt.index."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mcpnet_train_ref as ref          # noqa: E402

from learn_region_grow_amd import checkpoint, mcpnet_train      # noqa: E402

f64 = np.float64


def tie_free_case(seed, B=12, groups=3):
    rs = np.random.RandomState(seed)
    fc4 = rs.randn(B, 10) * 0.7
    labels = np.arange(B) % groups
    return fc4, labels


def closest_candidates(D, labels, margin=1.0):
    """The smallest gap that could flip a decision of the loss: two distances of a row, or a pair's term and zero."""
    gap = np.inf
    S, _ = ref.mine(D, labels)
    for a in range(len(D)):
        d = np.sort(np.delete(D[a], a))
        gap = min(gap, np.diff(d).min())
        for p in np.nonzero((labels == labels[a]) & (np.arange(len(D)) != a))[0]:
            gap = min(gap, abs(margin + D[a, p] - S[a, p]))
    return gap


def loss_of(fc4, labels):
    return ref.loss_forward(ref.pairwise_sq(ref.normalize(fc4), f64), labels)[0]


def twin_gradient(fc4, labels):
    emb = ref.normalize(fc4)
    lb = ref.loss_backward(ref.pairwise_sq(emb, f64), labels)
    return ref.l2_backward(fc4, ref.emb_grad(lb['dD'], emb)), lb


@pytest.mark.parametrize('seed,B,groups', [(1, 12, 3), (2, 12, 4), (3, 10, 2), (4, 9, 3)])
def test_backward_against_central_differences(seed, B, groups):
    fc4, labels = tie_free_case(seed, B, groups)
    assert closest_candidates(ref.pairwise_sq(ref.normalize(fc4), f64), labels) > 1e-6
    got, lb = twin_gradient(fc4, labels)
    assert lb['loss'] == pytest.approx(loss_of(fc4, labels), rel=1e-13)
    assert lb['active'] > 0
    h = 1e-7
    num = np.zeros_like(fc4)
    for i in range(B):
        for e in range(10):
            up, dn = fc4.copy(), fc4.copy()
            up[i, e] += h
            dn[i, e] -= h
            num[i, e] = (loss_of(up, labels) - loss_of(dn, labels)) / (2 * h)
    assert np.abs(got - num).max() <= 1e-6 * max(1.0, np.abs(num).max())


def torch_loss(fc4, labels, margin=1.0):
    """The graph of :157-236 in torch (float64) on amin / amax, whose gradients share equally among ties as TensorFlow's do."""
    import torch
    B = fc4.shape[0]
    emb = fc4 * torch.rsqrt(torch.clamp((fc4 * fc4).sum(1, keepdim=True), min=1e-12))
    sq = (emb * emb).sum(1, keepdim=True)
    D = torch.clamp(sq + sq.t() - 2.0 * emb @ emb.t(), min=0.0) * (1 - torch.eye(B, dtype=fc4.dtype))
    lab = torch.as_tensor(labels).view(B, 1)
    adj = lab == lab.t()
    adj_not = (~adj).to(fc4.dtype)
    tile = D.repeat(B, 1)
    mask = (~adj).repeat(B, 1) & (tile > D.t().reshape(-1, 1))
    mask_final = (mask.sum(1) > 0).view(B, B).t()
    hi = tile.amax(1, keepdim=True)
    outside = (((tile - hi) * mask.to(fc4.dtype)).amin(1, keepdim=True) + hi).view(B, B).t()
    lo = D.amin(1, keepdim=True)
    inside = (((D - lo) * adj_not).amax(1, keepdim=True) + lo).repeat(1, B)
    semi = torch.where(mask_final, outside, inside)
    pos = adj.to(fc4.dtype) - torch.eye(B, dtype=fc4.dtype)
    return torch.clamp((margin + (D - semi)) * pos, min=0.0).sum() / pos.sum()


@pytest.mark.parametrize('seed,B,groups', [(1, 12, 3), (5, 16, 4)])
def test_backward_against_torch_autograd(seed, B, groups):
    import torch
    fc4, labels = tie_free_case(seed, B, groups)
    assert closest_candidates(ref.pairwise_sq(ref.normalize(fc4), f64), labels) > 1e-6
    x = torch.tensor(fc4, dtype=torch.float64, requires_grad=True)
    loss = torch_loss(x, labels)
    loss.backward()
    got, lb = twin_gradient(fc4, labels)
    assert lb['loss'] == pytest.approx(float(loss.detach()), rel=1e-12)
    np.testing.assert_allclose(got, x.grad.numpy(), rtol=0, atol=1e-12)


# ---- constructed cases, worked out by hand ----
def unit(*xy):
    e = np.zeros(10)
    e[:len(xy)] = xy
    return e


def test_two_points_with_one_label():
    """D01 = 2; no negatives: both pairs take negatives_inside = 0; loss = (2 (1 + 2)) / 2; each pair sends 1 / 2 to its own distance."""
    D = ref.pairwise_sq(np.array([unit(1, 0), unit(0, 1)]), f64)
    lb = ref.loss_backward(D, np.array([7, 7]))
    assert D[0, 1] == 2 and lb['loss'] == 3 and lb['num_positives'] == 2 and lb['active'] == 2 and lb['fallback'] == 2
    assert np.array_equal(lb['dD'], [[0, 0.5], [0.5, 0]])


def test_all_labels_equal():
    """Four orthogonal unit rows: every distance 2, 12 positives, every pair 1 + 2 - 0, dD = 1 / 12 off the diagonal."""
    D = ref.pairwise_sq(np.eye(4, 10), f64)
    lb = ref.loss_backward(D, np.zeros(4, int))
    assert lb['loss'] == 3 and lb['num_positives'] == 12 and lb['fallback'] == 12
    assert np.array_equal(lb['dD'], (1 - np.eye(4)) / 12)
    assert ref.loss_forward(D, np.zeros(4, int))[0] == 3


def test_all_labels_distinct():
    D = ref.pairwise_sq(np.eye(4, 10), f64)
    lb = ref.loss_backward(D, np.arange(4))
    assert lb['num_positives'] == 0 and lb['active'] == 0 and np.isnan(lb['loss']) and not lb['dD'].any()
    assert np.isnan(ref.loss_forward(D, np.arange(4))[0])


HAND_ROWS = np.array([unit(1, 0), unit(0.8, 0.6), unit(0.6, 0.8), unit(0.6, 0.8)])
HAND_DD = np.array([[0, 0.25, -0.125, -0.125], [0.25, 0, -0.125, -0.125], [0, -0.25, 0, 0], [0, -0.25, 0, 0]])


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('labels', [[0, 0, 1, 1], [-5, -5, 2 ** 31 - 1, 2 ** 31 - 1], [-2 ** 31, -2 ** 31, -1, -1]])
def test_two_identical_rows_share_in_halves(dtype, labels):
    """Rows 2 and 3 are one point of the other label; D01 = 0.4, D02 = D03 = 0.8, D12 = D13 = 0.08, D23 = 0, g = 1 / 4.
      (0, 1): both negatives lie farther and tie: S = 0.8, term 0.6, - g / 2 to each; the row maximum (the same two) gets
              (- g + 2 g / 2) / 2 = 0
      (1, 0): no negative lies farther: negatives_inside = 0.08 (a tie again), term 1.32, - g / 2 to each
      (2, 3) and (3, 2): D = 0; the nearest farther negative is row 1 (0.08): term 0.92, - g to D21 and D31; the pair's own + g falls
              on a zero distance and dies in pairwise_distance's error mask
    Labels below zero and at the ends of int32 change nothing."""
    lab = np.array(labels, dtype=np.int64).astype(np.int32)
    D = ref.pairwise_sq(HAND_ROWS, dtype)
    assert D[0, 2] == D[0, 3] and D[2, 3] == 0
    lb = ref.loss_backward(D, lab)
    assert np.array_equal(lb['dD'], HAND_DD.astype(dtype))
    assert (lb['num_positives'], lb['active'], lb['fallback']) == (4, 4, 1)
    assert lb['loss'] == pytest.approx((0.6 + 1.32 + 0.92 + 0.92) / 4, rel=1e-6)
    assert ref.loss_forward(D, lab)[0] == pytest.approx(lb['loss'], rel=1e-12)


def test_the_only_farther_negative_is_the_row_maximum():
    """Row 0: D01 = 0.4 (positive), D02 = 0.08 (a nearer negative), D03 = 0.8 (the only farther one and the row's maximum).  The
    shifted minimum is 0 and ties with the three entries outside the mask: D03 gets - g / 4 from reduce_min and, as the row
    maximum, (- g + g / 4) / 1 from the two uses of axis_maximums: - g = - 1 / 4 in all."""
    rows = np.array([unit(1, 0), unit(0.8, 0.6), unit(0.96, 0.28), unit(0.6, 0.8)])
    D = ref.pairwise_sq(rows, f64)
    assert D[0, 2] < D[0, 1] < D[0, 3] == D[0].max()
    lb = ref.loss_backward(D, np.array([0, 0, 1, 1]))
    assert np.array_equal(lb['dD'][0], [0, 0.25, 0, -0.25])
    S, mf = ref.mine(D, np.array([0, 0, 1, 1]))
    assert mf[0, 1] and S[0, 1] == D[0, 3]


# ---- the checkpoint ----
def test_checkpoint_names_are_the_shipped_index(tmp_path):
    want = json.load(open(os.path.join(GOLDEN, 'mcpnet_model5_names.json')))
    w = mcpnet_train.initial_weights(3)
    t = checkpoint.mcpnet_checkpoint_tensors(w, step=7)
    got = [[k, list(np.shape(t[k])), np.asarray(t[k]).dtype.name] for k in sorted(t, key=lambda n: n.encode('utf-8'))]
    assert got == want and len(got) == 27
    assert int(t['Variable']) == 7
    prefix = str(tmp_path / 'mcpnet_model9.ckpt')
    checkpoint.write_bundle(prefix, t)
    back = checkpoint.load_mcpnet_weights(prefix)
    assert all(np.array_equal(back[k], w[k]) for k in w) and set(back) == set(w)
    with pytest.raises(KeyError):
        checkpoint.mcpnet_checkpoint_tensors({k: v for k, v in w.items() if k != 'mcp_bias4'})


def test_the_batch_limit_is_the_librarys(hip_lib):
    """mcpnet_train.MAX_BATCH restates LRG_MCP_TRIPLET_MAX_B: the library sizes a workspace up to it and refuses the next size."""
    import re
    from conftest import REPO
    header = open(os.path.join(REPO, 'include', 'lrg_hip.h')).read()
    assert int(re.search(r'#define\s+LRG_MCP_TRIPLET_MAX_B\s+(\d+)', header).group(1)) == mcpnet_train.MAX_BATCH
    assert hip_lib.lrg_mcp_triplet_workspace_doubles(mcpnet_train.MAX_BATCH) == 4 * mcpnet_train.MAX_BATCH
    assert hip_lib.lrg_mcp_triplet_workspace_doubles(mcpnet_train.MAX_BATCH + 1) == 0
    assert hip_lib.lrg_mcp_triplet_workspace_doubles(1) == 0


def test_initial_weights():
    w = mcpnet_train.initial_weights(0)
    assert {k: v.shape for k, v in w.items()} == checkpoint.MCPNET_SHAPES
    assert not w['mcp_bias3'].any() and w['mcp_kernel3'].dtype == np.float32
    assert np.abs(w['mcp_kernel1']).max() <= np.sqrt(6.0 / 206) and np.abs(w['mcp_kernel4']).max() <= np.sqrt(6.0 / 210)


# ---- batches and metrics ----
def test_even_sampling():
    rs = np.random.RandomState(0)
    labels = rs.permutation(np.repeat(np.arange(8), [200, 100, 80, 60, 40, 20, 9, 3]))
    assert len(labels) == 512
    idx = mcpnet_train.even_sampling(labels, 256, 16, np.random.RandomState(1))
    assert len(idx) == 256 and len(set(idx)) == 256 and min(idx) >= 0 and max(idx) < 512
    # the same state gives the same draw
    assert idx == mcpnet_train.even_sampling(labels, 256, 16, np.random.RandomState(1))
    # a visit takes 16 points of an instance, or all that is left of it: every instance gave a multiple of 16 or all its points,
    # but for the one whose visit the cut at 256 shortened
    taken = {int(v): int(n) for v, n in zip(*np.unique(labels[idx], return_counts=True))}
    have = {int(v): int(n) for v, n in zip(*np.unique(labels, return_counts=True))}
    assert sum(n % 16 != 0 and n != have[v] for v, n in taken.items()) <= 1
    # a block with fewer points than the batch: everything, once
    few = mcpnet_train.even_sampling(labels[:40], 256, 16, np.random.RandomState(2))
    assert sorted(few) == list(range(40))


def test_even_sampling_takes_at_most_sixteen_a_visit():
    labels = np.repeat([4, 9], [40, 40])
    st = np.random.RandomState(3)
    idx = mcpnet_train.even_sampling(labels, 32, 16, st)
    lab = labels[idx]
    assert len(idx) == 32 and len(set(idx)) == 32
    assert len(set(lab[:16])) == 1 and len(set(lab[16:])) == 1


def test_metrics_on_a_hand_case():
    """Two groups on a line: 0, 1 | 10, 11 and a stray 2.4 of the second group, whose nearest point belongs to the first."""
    emb = np.array([[0.0], [1.0], [10.0], [11.0], [2.4]])
    lb = np.array([3, 3, 8, 8, 8])
    assert mcpnet_train.nn_accuracy(emb, lb) == 4 / 5
    bg, wg, F = mcpnet_train.anova(emb, lb)
    # means 0.5 and 7.8, overall 4.88: between = (2 * 4.38^2 + 3 * 2.92^2) / 1, within = (0.25 + 0.25 + 2.2^2 + 3.2^2 + 5.4^2) / 3
    assert bg == pytest.approx(2 * 4.38 ** 2 + 3 * 2.92 ** 2) and wg == pytest.approx((0.25 + 0.25 + 2.2 ** 2 + 3.2 ** 2 + 5.4 ** 2) / 3)
    assert F == pytest.approx(bg / wg)
    assert mcpnet_train.anova(np.array([[1.0], [1.0], [2.0], [2.0]]), np.array([0, 0, 1, 1]))[2] == 0


def test_the_float64_restatement_learns():
    """LEARN_STEPS steps at batch LEARN_BATCH on four staged blocks of a synthetic room: the mean loss of the last third is below half
    of the first third's (0.59 -> 0.17 here), and the held-out block's nearest-neighbour accuracy does not fall (0.9375 -> 0.949)."""
    blocks = ref.learning_set()
    assert blocks[0].shape == (5, 512, 4) and blocks[1].shape == (5, 512, 50, 6) and blocks[2].shape == (5, 512)
    batches, held = ref.learning_batches(blocks, mcpnet_train.even_sampling)
    w0 = mcpnet_train.initial_weights(0)
    losses, w1 = ref.train_ref(w0, batches)
    third = ref.LEARN_STEPS // 3
    assert np.mean(losses[-third:]) < 0.5 * np.mean(losses[:third])
    acc0 = mcpnet_train.nn_accuracy(ref.forward(w0, held[1], held[0])['emb'], held[2])
    acc1 = mcpnet_train.nn_accuracy(ref.forward(w1, held[1], held[0])['emb'], held[2])
    assert acc1 >= acc0
