"""GPU: MCPNet (learn_region_grow_amd.mcpnet, csrc/lrg_mcpnet.hip, lrg_baseline_segment_embedding) against the reference's own draws,
embeddings and labels (tests/golden/mcpnet_ref_cpu.npz, made by tests/golden/make_mcpnet_golden.py) and the NumPy restatement
(tests/mcpnet_ref.py): exact integer paths, the network within the standing bound, repeatability, batching, errors and the CLI."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO
import mcpnet_ref as R

pytestmark = pytest.mark.gpu
ROOMS = (0, 1, 2)


def within(got, want):
    want = np.asarray(want, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - want) <= 1e-4 + 1e-5 * np.abs(want)


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'mcpnet_ref_cpu.npz'))


@pytest.fixture(scope='module')
def weights():
    z = np.load(os.path.join(GOLDEN, 'mcpnet_model5_weights.npz'))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def net(cuda_device, weights):
    from learn_region_grow_amd import mcpnet
    return mcpnet.MCPNetHIP(weights, device=cuda_device)


@pytest.fixture(scope='module')
def raw_rooms(golden):
    raw = R.golden_rooms(tuple(int(s) for s in golden['seeds']))
    assert R.rooms_digest(raw) == str(golden['rooms_digest'])
    return raw


@pytest.fixture(scope='module')
def rooms(cuda_device, raw_rooms):
    from learn_region_grow_amd import mcpnet
    return [mcpnet.prepare_room(r, room_id=k, device=cuda_device) for k, r in enumerate(raw_rooms)]


def test_preparation_equals_restatement(rooms, raw_rooms):
    for k, r in enumerate(rooms):
        p, eq, uq = R.equalize(R.center(raw_rooms[k]))
        assert np.array_equal(r['points'], p) and np.array_equal(r['equalized_idx'], eq) and np.array_equal(r['unequalized_idx'], uq)


def test_counts_and_legacy_neighbors_equal_reference(golden, rooms, cuda_device):
    from learn_region_grow_amd import mcpnet
    nbrs, counts = mcpnet.neighbors(rooms, rng='legacy', seed=0, device=cuda_device, return_counts=True)
    for r in ROOMS:
        assert np.array_equal(counts[r], golden['counts%d' % r]), r
        assert np.array_equal(nbrs[r][:256], golden['nbr_head%d' % r]), r
    assert R.nbr_digest(nbrs) == str(golden['nbr_digest'])
    # the state carries over: room by room with one RandomState gives the same draws
    state = np.random.RandomState(0)
    one = [mcpnet.neighbors([rooms[r]], rng='legacy', state=state, device=cuda_device)[0] for r in ROOMS]
    assert R.nbr_digest(one) == str(golden['nbr_digest'])


def test_counter_neighbors_equal_restatement_and_ignore_batching(rooms, cuda_device):
    from learn_region_grow_amd import mcpnet
    nbrs = mcpnet.neighbors(rooms, rng='counter', seed=7, device=cuda_device)
    for r in ROOMS:
        want = R.counter_neighbors(R.candidates(rooms[r]['points']), 7, rooms[r]['room_id'])
        assert np.array_equal(nbrs[r], want), r
        alone = mcpnet.neighbors([rooms[r]], rng='counter', seed=7, device=cuda_device)[0]
        assert np.array_equal(alone, nbrs[r]), r
    assert not np.array_equal(mcpnet.neighbors(rooms[:1], rng='counter', seed=8, device=cuda_device)[0], nbrs[0])


def test_network_layers_and_golden_embeddings(golden, rooms, net, weights, cuda_device):
    from learn_region_grow_amd import mcpnet
    nbrs = mcpnet.neighbors(rooms, rng='legacy', seed=0, device=cuda_device)
    embs = net.embed([r['points'] for r in rooms], nbrs)
    for r in ROOMS:
        f = R.forward(weights, rooms[r]['points'], nbrs[r])
        assert within(embs[r], f['emb']).all(), r
        assert within(embs[r], golden['emb%d' % r]).all(), r


def test_end_to_end_labels_equal_reference(golden, rooms, net, cuda_device):
    from learn_region_grow_amd import mcpnet
    nbrs = mcpnet.neighbors(rooms, rng='legacy', seed=0, device=cuda_device)
    embs = net.embed([r['points'] for r in rooms], nbrs)
    margin = float(golden['margin'])
    for r in ROOMS:
        # the stage that would move first: every 26-neighbour dot within half the stored margin of the reference's
        _, _, d_gpu = R.edge_pairs(rooms[r]['points'], embs[r])
        _, _, d_ref = R.edge_pairs(rooms[r]['points'], golden['emb%d' % r])
        assert np.abs(d_gpu - d_ref).max() < margin / 2, r
    labels = mcpnet.segment(rooms, embs, device=cuda_device)
    for r in ROOMS:
        assert np.array_equal(labels[r], golden['label%d' % r]), r
    # the clustering alone, from the reference's own embeddings
    labels = mcpnet.segment(rooms, [golden['emb%d' % r] for r in ROOMS], device=cuda_device)
    for r in ROOMS:
        assert np.array_equal(labels[r], golden['label%d' % r]), r


def test_repeatable_and_batch_independent(rooms, net, cuda_device):
    from learn_region_grow_amd import mcpnet
    nbrs = mcpnet.neighbors(rooms, rng='counter', seed=1, device=cuda_device)
    a = net.embed([r['points'] for r in rooms], nbrs)
    b = net.embed([r['points'] for r in rooms], nbrs)
    for r in ROOMS:
        assert a[r].tobytes() == b[r].tobytes()
        assert net.embed(rooms[r]['points'], nbrs[r]).tobytes() == a[r].tobytes()
    la = mcpnet.segment(rooms, a, device=cuda_device)
    for r in ROOMS:
        assert np.array_equal(mcpnet.segment([rooms[r]], [a[r]], device=cuda_device)[0], la[r])


@pytest.mark.parametrize('n', [1, 15, 16, 17, 33])
def test_point_counts_around_the_tile(n, rooms, net, weights, cuda_device):
    rs = np.random.RandomState(n)
    pts = rooms[0]['points'][:max(n, 1)]
    nbr = rs.randint(0, n, (n, 50))
    emb = net.embed(pts, nbr)
    assert emb.shape == (n, 10)
    assert within(emb, R.forward(weights, pts, nbr)['emb']).all()


def test_room_with_few_candidates(net, weights, cuda_device):
    from learn_region_grow_amd import mcpnet
    # points on a 1 m lattice: every point sees only itself and at most a few others (count < 50 everywhere)
    g = np.stack(np.meshgrid(np.arange(6), np.arange(5), np.arange(3), indexing='ij'), -1).reshape(-1, 3).astype(np.float32)
    rs = np.random.RandomState(2)
    raw = np.concatenate([g, rs.uniform(0, 1, (len(g), 3)).astype(np.float32)], axis=1)
    room = mcpnet.prepare_room(raw, room_id=4, device=cuda_device)
    for rng in ('legacy', 'counter'):
        nbrs, counts = mcpnet.neighbors([room], rng=rng, seed=3, device=cuda_device, return_counts=True)
        cands = R.candidates(room['points'])
        assert np.array_equal(counts[0], [len(c) for c in cands]) and counts[0].max() < 50
        want = R.legacy_neighbors(cands, np.random.RandomState(3)) if rng == 'legacy' else R.counter_neighbors(cands, 3, 4)
        assert np.array_equal(nbrs[0], want), rng
        emb = net.embed(room['points'], nbrs[0])
        assert within(emb, R.forward(weights, room['points'], nbrs[0])['emb']).all()


def pair_with_dot(target):
    """float32 rows a, b (dim 3) whose sequential float64 dot is exactly `target` (near 0.9): a = (f32(target), c1, c2), b = (1, 1, 1)."""
    a0 = np.float32(target)
    c1 = np.float32(target - float(a0))
    c2 = np.float32(target - float(a0) - float(c1))
    a = np.array([a0, c1, c2], np.float32)
    b = np.ones(3, np.float32)
    assert R.seq_dot(a[None], b[None])[0] == target
    return a, b


def test_embedding_predicate_boundaries(cuda_device):
    from learn_region_grow_amd import mcpnet
    # two points in neighbouring voxels; the dot of their embeddings decides the one edge
    pts = np.array([[0, 0, 0, 0, 0, 0], [0.1, 0, 0, 0, 0, 0]], dtype=np.float32)
    room = dict(points=pts)

    def edge(a, b, t=0.9):
        lab = mcpnet.segment([room], [np.stack([a, b])], threshold=t, min_cluster_size=1, device=cuda_device)[0]
        return bool(lab[0] == lab[1] == 1)
    assert not edge(*pair_with_dot(0.9))                          # a dot of exactly 0.9: no edge (strictly greater)
    assert edge(*pair_with_dot(np.nextafter(0.9, 1.0)))           # the next double above: an edge
    # a pair whose sequential sum and pairwise sum fall on either side of 0.9
    rs = np.random.RandomState(0)
    found = None
    for _ in range(200000):
        a = rs.randn(10).astype(np.float32)
        b = rs.randn(10).astype(np.float32)
        pr = a.astype(np.float64) * b.astype(np.float64)
        seq = R.seq_dot(a[None], b[None])[0]
        pair = ((pr[0] + pr[1]) + (pr[2] + pr[3])) + ((pr[4] + pr[5]) + (pr[6] + pr[7])) + (pr[8] + pr[9])
        if seq != pair:
            t = min(seq, pair) + (max(seq, pair) - min(seq, pair)) / 2
            if min(seq, pair) < t < max(seq, pair):
                found = (a, b, seq, t)
                break
    assert found is not None
    a, b, seq, t = found
    lab = mcpnet.segment([room], [np.stack([b, a])], threshold=t, min_cluster_size=1, device=cuda_device)[0]
    assert (lab[0] == lab[1] == 1) == (seq > t)


def test_large_scene_counter_mode(cuda_device, net):
    from learn_region_grow_amd import mcpnet, synthetic
    raw = synthetic.area5_shaped_room(200000, 9100).astype(np.float32)
    room = mcpnet.prepare_room(raw, room_id=0, device=cuda_device)
    assert len(room['points']) > 100000
    nbr = mcpnet.neighbors([room], rng='counter', seed=0, device=cuda_device)[0]
    assert nbr.min() >= 0 and nbr.max() < len(room['points'])
    emb = net.embed(room['points'], nbr)
    lab = mcpnet.segment([room], [emb], device=cuda_device)[0]
    assert np.array_equal(lab, R.components(room['points'], emb))


def test_errors(cuda_device, net, hip_lib, weights):
    from learn_region_grow_amd import _lib, mcpnet
    lib = hip_lib
    assert lib.lrg_mcp_workspace_bytes(-1, 1) == 0 and lib.lrg_mcp_workspace_bytes(10, 0) == 0
    assert lib.lrg_mcp_packed_floats() == 89416
    rs = (ctypes.c_int32 * 2)(0, 5)
    assert lib.lrg_mcp_candidates(None, 6, rs, 1, None, 0, None, None) != 0
    bad = (ctypes.c_int32 * 3)(0, 5, 3)
    assert lib.lrg_mcp_candidates(None, 6, bad, 2, None, 0, None, None) != 0
    assert lib.lrg_mcp_embed(None, 6, 4, None, None, None, None, None) != 0
    assert lib.lrg_mcp_embed(None, 6, -1, None, None, None, None, None) != 0
    assert lib.lrg_mcp_pack_weights(*([None] * 10)) != 0
    assert lib.lrg_baseline_segment(None, 6, rs, 1, ctypes.c_float(0.1), 5, None, None, None, 0.0, 0.0, 0.0, 10, None, 0, None, None, None) != 0
    assert lib.lrg_baseline_segment_embedding(None, 6, rs, 1, ctypes.c_float(0.1), None, 10, 0.9, 10, None, 0, None, None, None) != 0
    with pytest.raises(ValueError):
        mcpnet.neighbors([dict(points=np.zeros((2, 6), np.float32))], rng='other')
    with pytest.raises(ValueError):
        mcpnet.MCPNetHIP({k: (np.zeros((3,), np.float32) if k == 'mcp_bias1' else v) for k, v in weights.items()})
    # a neighbour index outside the room is reported, not read
    pts = np.zeros((3, 6), np.float32)
    with pytest.raises(_lib.LrgHipError):
        net.embed(pts, np.full((3, 50), 3))
    # a cell outside the window
    far = np.zeros((2, 6), np.float32)
    far[1, 0] = 1e6
    with pytest.raises(_lib.LrgHipError):
        mcpnet.neighbors([dict(points=far)], device=cuda_device)
    with pytest.raises(ValueError):
        mcpnet.segment([dict(points=pts)], [np.zeros((2, 10), np.float32)], device=cuda_device)


def test_cli(tmp_path, golden, raw_rooms, weights, rooms):
    from learn_region_grow_amd import checkpoint, io, metrics
    h5 = str(tmp_path / 'rooms.h5')
    io.saveToH5(h5, raw_rooms)
    ck = str(tmp_path / 'm' / 'mcp.ckpt')
    checkpoint.write_bundle(ck, weights)
    out = tmp_path / 'out'
    p = subprocess.run([sys.executable, os.path.join(REPO, 'mcpnet.py'), '--h5', h5, '--area', '5', '--ckpt', ck, '--save', str(out)],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.rstrip('\n').split('\n')
    assert lines[0] == 'Restored from %s' % ck
    assert [l for l in lines if l.startswith('Area ')] == [str(x) for x in golden['room_lines']]
    assert lines[-1] == str(golden['aggregate_line'])
    for r in ROOMS:
        obj = raw_rooms[r][rooms[r]['equalized_idx'], 6].astype(int)
        lab = golden['label%d' % r].astype(np.int64)
        cl2 = R.room_metrics(obj, lab)[3]
        emb_ply = (out / 'embedding' / ('%d.ply' % r)).read_text()
        res_ply = (out / 'results' / ('%d.ply' % r)).read_text()
        _, want_res = R.ply_points(rooms[r]['centred'], rooms[r]['unequalized_idx'], golden['emb%d' % r], cl2)
        assert res_ply == R.ply_text(want_res), r
        assert emb_ply.split('end_header\n')[0] == R.ply_text(want_res).split('end_header\n')[0]
        # the embedding colours come from a PCA of the GPU embeddings: positions exact, colours within one step of the golden's
        got = np.array([l.split() for l in emb_ply.split('end_header\n')[1].strip().split('\n')], dtype=np.float64)
        want_emb, _ = R.ply_points(rooms[r]['centred'], rooms[r]['unequalized_idx'], golden['emb%d' % r], cl2)
        assert np.array_equal(got[:, :3], np.array([[float('%f' % v) for v in q[:3]] for q in want_emb]))
        assert np.abs(got[:, 3:] - np.trunc(want_emb[:, 3:])).max() <= 1
