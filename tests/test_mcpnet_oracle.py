"""CPU: the NumPy restatement of test_mcpnet.py (tests/mcpnet_ref.py) against the reference script's own draws, embeddings, labels
and lines (tests/golden/mcpnet_ref_cpu.npz), the MCPNet weights fixture against the CRCs TensorFlow wrote, and the two RNG rules."""
import ctypes
import ctypes.util
import os

import numpy as np
import pytest

from conftest import GOLDEN
import mcpnet_ref as R
from learn_region_grow_amd import checkpoint as ck
from learn_region_grow_amd import mcpnet, metrics

ROOMS = (0, 1, 2)


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'mcpnet_ref_cpu.npz'))


@pytest.fixture(scope='module')
def weights():
    z = np.load(os.path.join(GOLDEN, 'mcpnet_model5_weights.npz'))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def rooms(golden):
    raw = R.golden_rooms(tuple(int(s) for s in golden['seeds']))
    assert R.rooms_digest(raw) == str(golden['rooms_digest'])
    out = []
    for r in raw:
        c = R.center(r)
        p, eq, uq = R.equalize(c)
        out.append(dict(raw=r, centred=c, points=p, eq=eq, uq=uq, obj=r[eq, 6].astype(int), cands=R.candidates(p)))
    return out


def test_weights_fixture_is_the_reference_checkpoint(weights):
    z = np.load(os.path.join(GOLDEN, 'mcpnet_bundle_small.npz'))
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, 'm.ckpt.index'), 'wb') as f:
            f.write(z['index'].tobytes())
        _, entries = ck.read_bundle_index(os.path.join(d, 'm.ckpt'))
    assert set(weights) == set(ck.MCPNET_SHAPES)
    for name, shp in ck.MCPNET_SHAPES.items():
        e = entries[name]
        a = weights[name]
        assert a.dtype == np.float32 and a.shape == shp == tuple(e.shape)
        assert ck.mask_crc(ck.crc32c(a.tobytes())) == e.crc32c, name


def test_load_mcpnet_weights_roundtrip(tmp_path, weights):
    extra = dict(weights)
    extra['mcp_kernel1/Adam'] = np.zeros((1, 6, 200), np.float32)
    extra['Variable'] = np.int32(7)
    prefix = str(tmp_path / 'mcp.ckpt')
    ck.write_bundle(prefix, extra)
    back = ck.load_mcpnet_weights(prefix)
    assert set(back) == set(ck.MCPNET_SHAPES)
    for k in back:
        assert np.array_equal(back[k], weights[k])
    bad = dict(weights)
    bad['mcp_kernel3'] = np.zeros((200, 200), np.float32)
    ck.write_bundle(str(tmp_path / 'bad.ckpt'), bad)
    with pytest.raises(ck.BundleError):
        ck.load_mcpnet_weights(str(tmp_path / 'bad.ckpt'))


@pytest.mark.parametrize('n', [1, 7, 49, 50, 51, 300])
def test_choice_of_list_is_list_of_choice(n):
    lst = list(range(1000, 1000 + 3 * n, 3))
    a, b = np.random.RandomState(5), np.random.RandomState(5)
    for _ in range(3):
        x = a.choice(lst, 50, replace=n < 50)
        y = np.asarray(lst)[b.choice(n, 50, replace=n < 50)]
        assert np.array_equal(x, y)
    assert np.array_equal(a.randint(0, 1 << 30, 8), b.randint(0, 1 << 30, 8))        # the same amount consumed
    # mcpnet.legacy_positions draws exactly this
    c, d = np.random.RandomState(9), np.random.RandomState(9)
    pos = mcpnet.legacy_positions(np.array([n, n]), c)
    assert np.array_equal(pos[0], d.choice(n, 50, replace=n < 50)) and np.array_equal(pos[1], d.choice(n, 50, replace=n < 50))


def test_length10_ddot_is_the_sequential_sum():
    rs = np.random.RandomState(3)
    a = rs.randn(20000, 10).astype(np.float32)
    b = rs.randn(20000, 10).astype(np.float32)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    dots = np.array([a64[i].dot(b64[i]) for i in range(len(a))])
    assert np.array_equal(dots, R.seq_dot(a, b))


def test_candidate_counts_and_legacy_draws_equal_reference(golden, rooms):
    state = np.random.RandomState(0)
    nbrs = []
    for r in ROOMS:
        cnt = np.array([len(c) for c in rooms[r]['cands']])
        assert np.array_equal(cnt, golden['counts%d' % r]), r
        nbrs.append(R.legacy_neighbors(rooms[r]['cands'], state))
        assert np.array_equal(nbrs[-1][:256], golden['nbr_head%d' % r]), r
    assert R.nbr_digest(nbrs) == str(golden['nbr_digest'])
    allc = np.concatenate([golden['counts%d' % r] for r in ROOMS])
    assert (allc < 50).any() and (allc >= 50).any()


def test_restated_network_within_tolerance(golden, rooms, weights):
    state = np.random.RandomState(0)
    for r in ROOMS:
        nbr = R.legacy_neighbors(rooms[r]['cands'], state)
        f = R.forward(weights, rooms[r]['points'], nbr)
        g = golden['emb%d' % r].astype(np.float64)
        assert np.all(np.abs(f['emb'] - g) <= 1e-4 + 1e-5 * np.abs(g)), r


def test_labels_and_lines_from_golden_embeddings(golden, rooms):
    ms = []
    for r in ROOMS:
        lab = R.components(rooms[r]['points'], golden['emb%d' % r])
        assert np.array_equal(lab, golden['label%d' % r]), r
        m = metrics.room_metrics_set_order(rooms[r]['obj'], lab)
        prc, rcl, iou, cl2 = R.room_metrics(rooms[r]['obj'], lab)
        assert np.array_equal(m['cluster_label2'], cl2)
        assert (m['rcl'], m['iou']) == (rcl, iou) and (m['prc'] == prc or (np.isnan(prc) and np.isnan(m['prc'])))
        assert metrics.room_line('5', r, m) == str(golden['room_lines'][r])
        ms.append(m)
    assert metrics.aggregate_line(ms) == str(golden['aggregate_line'])
    # the golden decides kept and dropped components, and no 26-neighbour dot is near the threshold
    assert max(int(golden['label%d' % r].max()) for r in ROOMS) > 0
    margin = min(float(np.abs(R.edge_pairs(rooms[r]['points'], golden['emb%d' % r])[2] - 0.9).min()) for r in ROOMS)
    assert margin == pytest.approx(float(golden['margin'])) and margin >= 1e-5


def test_set_order_metrics_differ_from_largest_first():
    obj = np.array([5] * 3 + [2] * 6 + [9] * 4)
    lab = np.array([1] * 3 + [2] * 6 + [0] * 4)
    m = metrics.room_metrics_set_order(obj, lab)
    assert list(m['cluster_label2'][:9]) == [5] * 3 + [2] * 6         # matched clusters carry the instance id
    assert list(metrics.room_metrics(obj, lab)['cluster_label2'][:9]) != list(m['cluster_label2'][:9])


def test_counter_rule_is_independent_of_batching(rooms):
    cands = rooms[1]['cands']
    full = R.counter_neighbors(cands, 3, 17)
    for i in (0, 5, len(cands) - 1):
        assert np.array_equal(R.counter_neighbors([cands[i]], 3, 17)[0], full[0] if i == 0 else R.counter_neighbors(cands[i:i + 1], 3, 17)[0])
        pos = R.counter_positions(len(cands[i]), 3, 17, i)
        assert np.array_equal(cands[i][pos], full[i])
    # count >= 50: 50 distinct positions; count < 50: draws with replacement (not LrgNet's all-n-first rule)
    big = R.counter_positions(80, 1, 2, 3)
    assert len(set(big.tolist())) == 50 and big.max() < 80
    small = R.counter_positions(20, 1, 2, 3)
    assert small.max() < 20 and not np.array_equal(small[:20], np.arange(20))
    assert not np.array_equal(R.counter_positions(80, 1, 2, 4), big)           # the point index is in the counter
    assert not np.array_equal(R.counter_positions(80, 1, 3, 3), big)           # and the room in the key
