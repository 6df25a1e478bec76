"""GPU: training MCPNet (csrc/lrg_mcpnet_train.hip, learn_region_grow_amd/mcpnet_train.py, train_mcpnet.py) against the NumPy
restatement tests/mcpnet_train_ref.py, which tests/test_mcpnet_train_host.py checks on its own.

tests/golden/mcpnet_trainer_bits.json pins three steps' digests; a change that means to alter the arithmetic records it again on
the GPU with `python tests/test_gpu_mcpnet_train.py --record` and says so.
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mcpnet_train_ref as ref                       # noqa: E402
from test_gpu_pointnet_train import within           # noqa: E402
from trainer_helpers import adam_f32, bits           # noqa: E402

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
K = 50
PTS = 2                                              # LRG_MCP_TRAIN_POINTS: the points of one workgroup of lrg_mcp_embed_train
EINVAL = -1000
BITS_FILE = os.path.join(GOLDEN, 'mcpnet_trainer_bits.json')


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev_of(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def shipped_weights():
    with np.load(os.path.join(GOLDEN, 'mcpnet_model5_weights.npz')) as z:
        return {k: z[k] for k in ref.NAMES}


def random_weights(seed):
    from learn_region_grow_amd.mcpnet_train import initial_weights
    w = initial_weights(seed)
    rs = np.random.RandomState(seed + 50)
    for k in w:
        if 'bias' in k:
            w[k] = rs.uniform(-0.1, 0.1, w[k].shape).astype(f32)
    return w


def pack(lib, w, dev):
    import torch
    packed = torch.empty(lib.lrg_mcp_packed_floats(), dtype=torch.float32, device=dev)
    t = [dev_of(np.asarray(w[k], f32), dev) for k in ref.NAMES]
    assert lib.lrg_mcp_pack_weights(*[ptr(x) for x in t], ptr(packed), stream()) == 0
    torch.cuda.synchronize()
    return packed


def room_like(n, seed):
    """n points (x, y, z, r, g, b) and 50 neighbour indices each."""
    rs = np.random.RandomState(seed)
    pts = np.concatenate([rs.uniform(-0.4, 0.4, (n, 2)), rs.uniform(0, 2.5, (n, 1)), rs.uniform(0, 1, (n, 3))], axis=1).astype(f32)
    return pts, rs.randint(0, n, (n, K)).astype(np.int32)


# ---------------------------------------------------------------- the forward pass that keeps its layers ----------------------------------------------------------------
@pytest.mark.parametrize('weights', ['shipped', 'random'])
@pytest.mark.parametrize('n', sorted({1, PTS - 1, PTS, PTS + 1, 5, 256}))     # 5: several workgroups and an odd tail
def test_keep_forward(hip_lib, cuda_device, n, weights):
    import torch
    w = shipped_weights() if weights == 'shipped' else random_weights(n)
    pts, nbr = room_like(n, 10 + n)
    rows = pts[nbr, :6] - pts[:, None, :6]
    centre = np.ascontiguousarray(pts[:, 2:6])
    packed = pack(hip_lib, w, cuda_device)
    d_pts, d_nbr, d_x, d_c = (dev_of(a, cuda_device) for a in (pts, nbr, rows, centre))

    def out(*shape):
        return torch.full(shape, float('nan'), dtype=torch.float32, device=cuda_device)
    status = torch.zeros(1, dtype=torch.int32, device=cuda_device)
    want_emb = out(n, 10)
    assert hip_lib.lrg_mcp_embed(ptr(d_pts), 6, n, ptr(d_nbr), ptr(packed), ptr(want_emb), ptr(status), stream()) == 0
    h1, h2, cat, fc3, fc4, emb, emb2 = out(n * K, 200), out(n * K, 200), out(n, 204), out(n, 200), out(n, 10), out(n, 10), out(n, 10)
    assert hip_lib.lrg_mcp_embed_train(ptr(d_x), ptr(d_c), n, ptr(packed), ptr(h1), ptr(h2), ptr(cat), ptr(fc3), ptr(fc4), ptr(emb), stream()) == 0
    assert hip_lib.lrg_mcp_embed_train(ptr(d_x), ptr(d_c), n, ptr(packed), None, None, None, None, None, ptr(emb2), stream()) == 0
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    got = {k: v.cpu().numpy() for k, v in dict(h1=h1, h2=h2, cat=cat, fc3=fc3, fc4=fc4, emb=emb).items()}
    assert np.array_equal(bits(got['emb']), bits(want_emb.cpu().numpy()))
    assert np.array_equal(bits(emb2.cpu().numpy()), bits(got['emb']))
    assert np.array_equal(bits(got['cat'][:, 4:]), bits(got['h2'].reshape(n, K, 200).max(axis=1)))
    assert np.array_equal(bits(got['cat'][:, :4]), bits(centre))
    r64, r32 = ref.forward(w, rows, centre, f64), ref.forward(w, rows, centre, f32)
    for k in ('h1', 'h2', 'cat', 'fc3', 'fc4', 'emb'):
        within('%s n=%d %s' % (k, n, weights), got[k], r64[k], r32[k])


# ---------------------------------------------------------------- the loss ----------------------------------------------------------------
PATTERNS = ('sixteen', 'one-instance', 'all-distinct', 'singleton', 'duplicated-rows', 'clustered')


def loss_case(B, pattern):
    rs = np.random.RandomState(1000 * PATTERNS.index(pattern) + B)
    fc4 = (rs.randn(B, 10) * 0.8).astype(f32)
    if pattern == 'sixteen':
        labels = (np.arange(B) // 16) * 7919 - 2 ** 31           # from the lower end of int32 upwards
    elif pattern == 'one-instance':
        labels = np.full(B, 2 ** 31 - 1)
    elif pattern == 'all-distinct':
        labels = rs.permutation(B) - B // 2
    elif pattern == 'singleton':
        labels = np.arange(B) % 3
        labels[B // 2] = 77
    elif pattern == 'clustered':                                 # instances apart: many pairs keep their margin and send no gradient
        labels = (np.arange(B) // 4) % 8
        fc4 = (rs.randn(8, 10)[labels] + 0.15 * rs.randn(B, 10)).astype(f32)
    else:
        labels = np.arange(B) % 4
        half = max(1, B // 2)
        fc4 = fc4[np.arange(B) % half]                           # rows i and i + half are one point; their labels agree or not
    ss = (fc4 * fc4).sum(axis=1, keepdims=True)
    emb = fc4 * (f32(1) / np.sqrt(np.maximum(ss, f32(1e-12))))
    return np.ascontiguousarray(fc4), emb.astype(f32), labels.astype(np.int64).astype(np.int32)


def run_loss(lib, dev, fc4, emb, labels, margin=1.0):
    import torch
    B = len(labels)
    D = torch.full((B, B), float('nan'), dtype=torch.float32, device=dev)
    dD, dfc4 = torch.full_like(D, float('nan')), torch.full((B, 10), float('nan'), dtype=torch.float32, device=dev)
    stats = torch.zeros(4, dtype=torch.float64, device=dev)
    ws = torch.zeros(lib.lrg_mcp_triplet_workspace_doubles(B), dtype=torch.float64, device=dev)
    t = [dev_of(a, dev) for a in (fc4, emb, labels)]
    rc = lib.lrg_mcp_triplet_semihard(ptr(t[0]), ptr(t[1]), ptr(t[2]), B, ctypes.c_float(margin), ptr(D), ptr(dD), ptr(dfc4), ptr(stats), ptr(ws),
                                      stream())
    assert rc == 0
    torch.cuda.synchronize()
    return D.cpu().numpy(), dD.cpu().numpy(), dfc4.cpu().numpy(), stats.cpu().numpy()


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('B', [2, 3, 63, 64, 65, 256])
def test_loss_kernel(hip_lib, cuda_device, B, pattern):
    fc4, emb, labels = loss_case(B, pattern)
    D, dD, dfc4, stats = run_loss(hip_lib, cuda_device, fc4, emb, labels)
    D32 = ref.pairwise_sq(emb, f32)
    assert np.array_equal(bits(D), bits(D32))
    lb = ref.loss_backward(D32, labels)
    print('B %d %s: loss numerator %.9g (twin %.9g), positives %d, active %d, inside %d' %
          (B, pattern, stats[0], lb['numerator'], stats[1], stats[2], stats[3]))
    assert np.array_equal(bits(dD), bits(lb['dD']))
    assert (int(stats[1]), int(stats[2]), int(stats[3])) == (lb['num_positives'], lb['active'], lb['fallback'])
    assert stats[0] == pytest.approx(lb['numerator'], rel=2e-5, abs=0)
    if pattern == 'clustered' and B >= 63:
        assert 0 < stats[2] < stats[1]
    if pattern == 'all-distinct':
        assert stats[1] == 0 and stats[0] == 0 and not dD.any() and not dfc4.any()
    # dfc4 against the float64 restatement given that dD
    want64 = ref.l2_backward(fc4.astype(f64), ref.emb_grad(dD.astype(f64), emb.astype(f64)))
    want32 = ref.l2_backward(fc4, ref.emb_grad(dD, emb))
    within('dfc4 B=%d %s' % (B, pattern), dfc4, want64, want32)
    again = run_loss(hip_lib, cuda_device, fc4, emb, labels)
    for a, b in zip((D, dD, dfc4), again[:3]):
        assert np.array_equal(bits(a), bits(b))
    assert np.array_equal(stats, again[3])


def test_loss_kernel_refuses_bad_sizes(hip_lib, cuda_device):
    import torch
    z = torch.zeros(16, dtype=torch.float32, device=cuda_device)
    i = torch.zeros(16, dtype=torch.int32, device=cuda_device)
    d = torch.full((8,), 7.0, dtype=torch.float64, device=cuda_device)
    from learn_region_grow_amd import mcpnet_train
    assert hip_lib.lrg_mcp_triplet_workspace_doubles(mcpnet_train.MAX_BATCH) == 4 * mcpnet_train.MAX_BATCH
    for B in (1, 0, -3, mcpnet_train.MAX_BATCH + 1):
        rc = hip_lib.lrg_mcp_triplet_semihard(ptr(z), ptr(z), ptr(i), B, ctypes.c_float(1.0), ptr(z), ptr(z), ptr(z), ptr(d), ptr(d), stream())
        assert EINVAL - 100 < rc < EINVAL
        assert hip_lib.lrg_mcp_triplet_workspace_doubles(B) == 0
    assert hip_lib.lrg_mcp_triplet_semihard(ptr(z), None, ptr(i), 2, ctypes.c_float(1.0), ptr(z), ptr(z), ptr(z), ptr(d), ptr(d), stream()) < EINVAL
    assert hip_lib.lrg_mcp_embed_train(None, ptr(z), 2, ptr(z), None, None, None, None, None, ptr(z), stream()) < EINVAL
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == 7.0).all() and not z.cpu().numpy().any()          # nothing was launched


# ---------------------------------------------------------------- the trainer ----------------------------------------------------------------
def batch(B, seed):
    """A batch shaped like a staged one: rows within the 0.3 m cells, centre features (z, r, g, b), 16 (B = 16: 4) points an instance."""
    rs = np.random.RandomState(seed)
    rows = np.concatenate([rs.uniform(-0.45, 0.45, (B, K, 3)), rs.uniform(-0.6, 0.6, (B, K, 3))], axis=2).astype(f32)
    inst = np.arange(B) // (4 if B == 16 else 16)
    centre = np.concatenate([rs.uniform(0, 2.5, (B, 1)), np.clip(0.5 + 0.3 * rs.randn(len(set(inst)), 3)[inst] + 0.05 * rs.randn(B, 3), 0, 1)],
                            axis=1).astype(f32)
    return centre, rows, rs.permutation(40)[inst].astype(np.int32)


def make_trainer(B, dev, weights=None):
    from learn_region_grow_amd.mcpnet_train import MCPNetTrainer
    return MCPNetTrainer(B, device=dev).load_weights(shipped_weights() if weights is None else weights)


@pytest.mark.parametrize('B', [16, 64, 256])
def test_trainer_gradients_and_update(cuda_device, B):
    """The eight gradients against the float64 restatement of sum(G * D(theta)) with G the device's own dD (float32 and float64 mining
    may pick different negatives; dD itself is proved bit-equal to the float32 restatement in test_loss_kernel), then the update
    against adam_f32 on the device's own gradients."""
    import torch
    w = shipped_weights()
    centre, rows, labels = batch(B, B)
    tr = make_trainer(B, cuda_device, w)
    with torch.cuda.device(cuda_device):
        tr.forward_backward(centre, rows, labels)
        torch.cuda.synchronize()
        G = tr._dD.cpu().numpy()
        D, emb = tr._D.cpu().numpy(), tr._emb.cpu().numpy()
        grads = tr.grads_numpy()
        p0, g0 = tr.flat.cpu().numpy(), tr.gflat.cpu().numpy()
    assert np.array_equal(bits(D), bits(ref.pairwise_sq(emb, f32)))
    assert np.array_equal(bits(G), bits(ref.loss_backward(D, labels)['dD']))
    assert G.any()
    _, g64, _ = ref.step_ref(w, rows, centre, G, f64)
    _, g32, _ = ref.step_ref(w, rows, centre, G, f32)
    for k in ref.NAMES:
        within('%s B=%d' % (k, B), grads[k], g64[k], g32[k])
    out = tr.train_step(centre, rows, labels)
    with torch.cuda.device(cuda_device):
        p1, g1, m1, v1 = (x.cpu().numpy() for x in (tr.flat, tr.gflat, tr.m, tr.v))
    assert np.array_equal(bits(g1), bits(g0)) and tr.step == 1 and np.isfinite(out['loss'])
    lr_t = ctypes.c_float(1e-3 * np.sqrt(1.0 - 0.999) / (1.0 - 0.9)).value
    wp, wm, wv = adam_f32(p0, g0, np.zeros_like(p0), np.zeros_like(p0), lr_t, 0.9, 0.999, 1e-8)
    assert np.array_equal(bits(p1), bits(wp)) and np.array_equal(bits(m1), bits(wm)) and np.array_equal(bits(v1), bits(wv))
    assert out['emb'].shape == (B, 10) and np.array_equal(bits(out['emb']), bits(emb))


def test_a_batch_without_positives_is_skipped(cuda_device):
    import torch
    centre, rows, _ = batch(16, 3)
    tr = make_trainer(16, cuda_device)
    with torch.cuda.device(cuda_device):
        before = tr.flat.cpu().numpy()
    out = tr.train_step(centre, rows, np.arange(16))
    with torch.cuda.device(cuda_device):
        after = tr.flat.cpu().numpy()
    assert np.isnan(out['loss']) and out['num_positives'] == 0 and tr.skipped_batches == 1 and tr.step == 0
    assert np.array_equal(bits(before), bits(after))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def three_steps(dev):
    """Digests of flat, m, v, gflat and float.hex of the losses after three steps at B = 64 from initial_weights(7)."""
    import torch
    from learn_region_grow_amd.mcpnet_train import initial_weights
    tr = make_trainer(64, dev, initial_weights(7))
    losses = []
    for step in range(3):
        centre, rows, labels = batch(64, 200 + step)
        losses.append(float(tr.train_step(centre, rows, labels)['loss']).hex())
    with torch.cuda.device(dev):
        out = {k: sha(getattr(tr, k).cpu().numpy()) for k in ('flat', 'm', 'v', 'gflat')}
    out['losses'] = losses
    return out


def test_three_steps_twice_and_the_recorded_bits(cuda_device):
    a, b = three_steps(cuda_device), three_steps(cuda_device)
    assert a == b
    assert a == json.load(open(BITS_FILE))['three_steps']


# ---------------------------------------------------------------- staging ----------------------------------------------------------------
def test_staging_matches_the_literal_loops(cuda_device, tmp_path):
    from learn_region_grow_amd import mcpnet_train, synthetic
    rooms = [synthetic.generate_room_points(3000, s).astype(f32) for s in (21, 22)]
    small = synthetic.generate_room_points(300, 23).astype(f32)
    st_a, st_b = np.random.RandomState(4), np.random.RandomState(4)
    want = []
    for r in (rooms[0], small, rooms[1]):
        got = ref.stage_room_ref(r[:, :6], r[:, 6].astype(np.int32), st_a)
        if got is not None:
            want.append(got)
    assert len(want) == 2
    lines = []
    staged = mcpnet_train.stage_area([(r[:, :6], r[:, 6].astype(np.int32)) for r in (rooms[0], small, rooms[1])], st_b, area=3,
                                     device=cuda_device, log=lines.append)
    assert len(lines) == 3 and 'skipped' in lines[1] and lines[0].startswith('AREA 3 room 0 ') and lines[0].endswith('%d batches' % len(want[0][0]))
    for k in range(3):
        w = np.concatenate([x[k] for x in want])
        assert staged[k].dtype == w.dtype and np.array_equal(staged[k], w)
    assert st_a.randint(1 << 30) == st_b.randint(1 << 30)                      # both streams stand at the same place
    path = str(tmp_path / 'data' / 'mcp_area3.h5')
    mcpnet_train.write_staged(path, *staged)
    back = mcpnet_train.read_staged(path)
    for k in range(3):
        assert back[k].dtype == staged[k].dtype and np.array_equal(back[k], staged[k])


# ---------------------------------------------------------------- learning ----------------------------------------------------------------
def test_it_learns_and_the_checkpoint_runs(cuda_device, tmp_path):
    """The steps of test_the_float64_restatement_learns on the device: the last third's mean loss is below the first third's and the
    held-out accuracy does not fall; then save -> load_mcpnet_weights -> MCPNetHIP.embed gives evaluate's embeddings bit for bit."""
    from learn_region_grow_amd import checkpoint, mcpnet_train
    from learn_region_grow_amd.mcpnet import MCPNetHIP
    batches, held = ref.learning_batches(ref.learning_set(), mcpnet_train.even_sampling)
    tr = mcpnet_train.MCPNetTrainer(ref.LEARN_BATCH, device=cuda_device).init_weights(0)
    acc0 = mcpnet_train.nn_accuracy(tr.evaluate(*held)['emb'], held[2])
    losses = [tr.train_step(*b)['loss'] for b in batches]
    ev = tr.evaluate(*held)
    acc1 = mcpnet_train.nn_accuracy(ev['emb'], held[2])
    third = ref.LEARN_STEPS // 3
    print('loss %.4f -> %.4f, held-out accuracy %.4f -> %.4f' % (np.mean(losses[:third]), np.mean(losses[-third:]), acc0, acc1))
    assert np.isfinite(losses).all() and tr.step == ref.LEARN_STEPS
    assert np.mean(losses[-third:]) < np.mean(losses[:third])
    assert acc1 >= acc0
    prefix = str(tmp_path / 'mcpnet_model7.ckpt')
    tr.save(prefix)
    net = MCPNetHIP(checkpoint.load_mcpnet_weights(prefix), device=cuda_device)
    # points whose float32 differences are the held-out rows: the centre at the origin, its 50 neighbours at the rows themselves
    n = 40
    p4, rows, lab = (a[:n] for a in held)
    pts = np.zeros((n * 51, 6), f32)
    pts[:n, 2:6] = p4
    pts[n:] = rows.reshape(-1, 6) + np.repeat(pts[:n], K, axis=0)
    x = pts[n:].reshape(n, K, 6) - pts[:n, None, :]
    nbr = np.zeros((n * 51, K), np.int32)
    nbr[:n] = n + np.arange(n * K).reshape(n, K)
    nbr[n:] = np.arange(n, n * 51)[:, None]
    emb = net.embed(pts, nbr)[:n]
    assert np.array_equal(bits(emb), bits(tr.evaluate(p4, x, lab)['emb']))


# ---------------------------------------------------------------- the command line ----------------------------------------------------------------
def test_command_line_stages_trains_and_the_checkpoint_runs(cuda_device, tmp_path):
    from learn_region_grow_amd import checkpoint, io, synthetic
    data = tmp_path / 'data'
    os.makedirs(str(data))
    for area, seeds in ((1, (31,)), (2, (32,))):
        io.saveToH5(str(data / ('s3dis_area%d.h5' % area)), [synthetic.generate_room_points(2000, s).astype(f32) for s in seeds])
    model = str(tmp_path / 'models' / 'mcpnet_model2.ckpt')
    env = dict(os.environ, PYTHONPATH=REPO)
    exe = [sys.executable, os.path.join(REPO, 'train_mcpnet.py'), '--data', str(data)]
    r = subprocess.run(exe + ['--stage', '--areas', '1,2'], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'AREA 1 room 0' in r.stdout and os.path.exists(str(data / 'mcp_area2.h5'))
    r = subprocess.run(exe + ['--area', '2', '--areas', '1,2', '--epochs', '1', '--model', model], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith('Epoch 0 loss ')]
    assert len(line) == 1
    words = line[0].split()
    assert words[::2] == ['Epoch', 'loss', 'acc', 'bg', 'wg', 'F'] and all(np.isfinite(float(x)) for x in words[1::2])
    assert set(checkpoint.load_mcpnet_weights(model)) == set(ref.NAMES)
    pts = synthetic.generate_room_points(1500, 33).astype(f32)
    room = str(tmp_path / 'room.h5')
    io.saveToH5(room, [pts])
    r = subprocess.run([sys.executable, os.path.join(REPO, 'mcpnet.py'), '--h5', room, '--area', '2', '--ckpt', model], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


if __name__ == '__main__':
    if '--record' not in sys.argv:
        sys.exit(__doc__)
    import torch
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else BITS_FILE
    with open(out, 'w') as f:
        json.dump({'recorded': 'python tests/test_gpu_mcpnet_train.py --record', 'three_steps': three_steps(torch.device('cuda:0'))}, f, indent=1,
                  sort_keys=True)
        f.write('\n')
    print('wrote', out)
