"""GPU: training batches drawn on the device (lrg_train_assemble, lrg_ce_grad_counted, train_data.TupleStore, LrgNetTrainer's device
entries, stage_rooms_gpu(download=False), train_region_grow.py --assemble device / --stage online) against the host twin
(tests/assemble_ref.py) and against the host path they replace.  Everything compared is a copy, an integer sum or the trainer's own
arithmetic on equal inputs, so every comparison is exact: no tolerance anywhere."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import assemble_ref
import stage_ref
from learn_region_grow_amd import _lib, stage, synthetic
from learn_region_grow_amd.lrgnet import _ptr, _stream_ptr
from learn_region_grow_amd.train_data import BatchBuffers, TupleStore

pytestmark = pytest.mark.gpu
K = 64
EINVAL = _lib.LRG_EINVAL


@pytest.fixture(scope='module')
def tuples():
    return assemble_ref.constructed_tuples()


@pytest.fixture(scope='module')
def store(cuda_device, tuples):
    up = {k: torch.from_numpy(tuples[k]).to(cuda_device) for k in ('points', 'remove', 'neighbor_points', 'add')}
    return TupleStore(up['points'], up['remove'], up['neighbor_points'], up['add'], tuples['start_in'], tuples['count_in'], tuples['start_nb'],
                      tuples['count_nb'], 13, rng_seed=5)


# ---------------------------------------------------------------- 1. assembly against the twin ----------------------------------------------------------------
@pytest.mark.parametrize('order', [[0, 1, 2, 3, 4, 5, 6, 7], [6, 1, 7]])
@pytest.mark.parametrize('F', [13, 6])
def test_assembly_equals_the_twin(cuda_device, tuples, store, order, F):
    st = store if F == 13 else TupleStore(store.points, store.remove, store.neighbor_points, store.add, store.start_in, store.count_in,
                                          store.start_nb, store.count_nb, F, rng_seed=5)
    bufs = BatchBuffers(len(order), K, K, F, cuda_device)
    d_order = st.upload_order(order)
    for pass_ in (0, 1):
        for epoch in (0, 3):
            want = assemble_ref.assemble_batch(tuples, order, K, K, F, 5, epoch, pass_)
            got = []
            for _ in range(2):
                for t in (bufs.inlier, bufs.neighbor, bufs.add, bufs.remove, bufs.positives_remove, bufs.positives_add):
                    t.fill_(-7)
                st.assemble(d_order, epoch, pass_, bufs)
                got.append([t.cpu().numpy() for t in (bufs.inlier, bufs.neighbor, bufs.add, bufs.remove, bufs.positives_remove, bufs.positives_add)])
            for name, g, g2, w in zip(('inlier', 'neighbor', 'add', 'remove', 'positives_remove', 'positives_add'), got[0], got[1], want):
                assert g.dtype == w.dtype and g.shape == w.shape, name
                assert g.tobytes() == w.tobytes(), (name, pass_, epoch)
                assert g.tobytes() == g2.tobytes(), name                       # the same call again: the same bytes
    # the constructed flags reach both ends of the count
    if len(order) == 8:
        assert got[0][4][2] == 0 and got[0][4][5] == K and got[0][5][2] == 0 and got[0][5][5] == K


def test_assembly_refuses_bad_arguments(cuda_device, hip_lib, store):
    bufs = BatchBuffers(3, K, K, 13, cuda_device)
    order = store.upload_order([6, 1, 7])
    t_start, t_count = store._tables[0], store._tables[1]

    def call(**kw):
        a = dict(rows=_ptr(store.points), stride=13, labels=_ptr(store.remove), start=_ptr(t_start), count=_ptr(t_count), order=_ptr(order), B=3, k=K,
                 F=13, out_rows=_ptr(bufs.inlier), out_labels=_ptr(bufs.remove), positives=_ptr(bufs.positives_remove))
        a.update(kw)
        return hip_lib.lrg_train_assemble(a['rows'], a['stride'], a['labels'], a['start'], a['count'], a['order'], a['B'], a['k'], a['F'], 5, 0, 0,
                                          _lib.LRG_PURPOSE_TRAIN_INLIER, a['out_rows'], a['out_labels'], a['positives'], _stream_ptr())
    bufs.inlier.fill_(-7)
    for name in ('rows', 'labels', 'start', 'count', 'order', 'out_rows', 'out_labels', 'positives'):
        assert call(**{name: None}) <= EINVAL, name
    codes = [call(B=0), call(k=0), call(F=0), call(F=14), call(stride=12)]
    assert all(c <= EINVAL for c in codes) and len(set(codes[:4])) == 4, codes
    assert call(k=_lib.LRG_ASSEMBLE_MAX_POINTS + 1) <= EINVAL
    torch.cuda.synchronize()
    assert bool((bufs.inlier == -7).all())                                     # refused before any launch
    assert call() == 0
    with pytest.raises(ValueError):
        store.upload_order([0, 8])
    with pytest.raises(ValueError):                                            # N >= 1 is checked on the host table
        TupleStore(store.points, store.remove, store.neighbor_points, store.add, store.start_in, store.count_in, store.start_nb,
                   np.array([3000, 1024, 129, 65, 64, 63, 2, 0], dtype=np.int32), 13)


# ---------------------------------------------------------------- 2. lrg_ce_grad_counted ----------------------------------------------------------------
@pytest.mark.parametrize('labels', ['mixed', 'zeros', 'ones'])
def test_counted_weights_give_the_host_weights_bits(cuda_device, hip_lib, labels):
    rows = 3 * K
    rs = np.random.RandomState(11)
    logits = (rs.randn(rows, 2) * 3).astype(np.float32)
    lab = {'mixed': rs.randint(0, 2, rows), 'zeros': np.zeros(rows), 'ones': np.ones(rows)}[labels].astype(np.int32)
    positives = lab.reshape(3, K).sum(axis=1).astype(np.int32)
    n_pos, n_neg = int(lab.sum()), int(rows - lab.sum())
    if labels == 'mixed':
        assert 0 < n_pos < rows and float(np.float32(1.0 / n_pos)) != 1.0 / n_pos      # a weight that float32 has to round
    dlg, dlab, dpos = torch.from_numpy(logits).to(cuda_device), torch.from_numpy(lab).to(cuda_device), torch.from_numpy(positives).to(cuda_device)
    out = []
    for counted in (False, True):
        dl = torch.full((rows, 2), -7.0, dtype=torch.float32, device=cuda_device)
        stats = torch.zeros(8, dtype=torch.float64, device=cuda_device)
        if counted:
            rc = hip_lib.lrg_ce_grad_counted(_ptr(dlg), _ptr(dlab), rows, _ptr(dpos), 3, _ptr(dl), _ptr(stats), _stream_ptr())
        else:
            rc = hip_lib.lrg_ce_grad(_ptr(dlg), _ptr(dlab), rows, 1.0 / n_pos if n_pos else 0.0, 1.0 / n_neg if n_neg else 0.0, _ptr(dl), _ptr(stats),
                                     _stream_ptr())
        assert rc == 0
        out.append((dl.cpu().numpy(), stats.cpu().numpy()))
    assert out[0][0].tobytes() == out[1][0].tobytes()
    assert out[0][1].tobytes() == out[1][1].tobytes()
    assert out[1][1][5] == rows and out[1][1][4] == n_pos and np.isfinite(out[1][0]).all()
    assert hip_lib.lrg_ce_grad_counted(_ptr(dlg), _ptr(dlab), rows, None, 3, _ptr(dl), _ptr(stats), _stream_ptr()) <= EINVAL
    assert hip_lib.lrg_ce_grad_counted(_ptr(dlg), _ptr(dlab), rows, _ptr(dpos), 0, _ptr(dl), _ptr(stats), _stream_ptr()) <= EINVAL


# ---------------------------------------------------------------- 3. the trainer ----------------------------------------------------------------
@pytest.mark.parametrize('lite,F', [(0, 13), (2, 12)])
def test_device_steps_equal_host_steps_on_the_twins_batches(cuda_device, tuples, store, lite, F):
    from learn_region_grow_amd.train import LrgNetTrainer
    B = 3
    st = store if F == 13 else TupleStore(store.points, store.remove, store.neighbor_points, store.add, store.start_in, store.count_in,
                                          store.start_nb, store.count_nb, F, rng_seed=5)
    w = synthetic.make_reference_init_weights(seed=1, feature_size=F, lite=lite)
    a = LrgNetTrainer(B, K, K, F, lite, device=cuda_device).load_weights(w)
    b = LrgNetTrainer(B, K, K, F, lite, device=cuda_device).load_weights(w)
    orders = [[6, 1, 7], [0, 5, 3], [2, 4, 6]]                                 # the second remove side is all 1 in one instance, the third all 0
    bufs = BatchBuffers(B, K, K, F, cuda_device)
    stats = torch.full((4, 2, 8), -1.0, dtype=torch.float64, device=cuda_device)
    d_order = st.upload_order(np.concatenate(orders))
    host_scalars = []
    for step, order in enumerate(orders):
        xi, xn, ia, ir, _, _ = assemble_ref.assemble_batch(tuples, order, K, K, F, 5, step, 0)
        host_scalars.append(a.train_step(xi, xn, ia, ir))
        st.assemble(d_order[step * B:(step + 1) * B], step, 0, bufs)
        assert b.train_step_device(bufs.inlier, bufs.neighbor, bufs.add, bufs.remove, bufs.positives_remove, stats[step]) is None
    # evaluation of one more batch, both ways, on the weights after the three steps
    xi, xn, ia, ir, _, _ = assemble_ref.assemble_batch(tuples, orders[0], K, K, F, 5, 9, 1)
    host_eval = a.evaluate(xi, xn, ia, ir)
    st.assemble(d_order[:B], 9, 1, bufs)
    b.evaluate_device(bufs.inlier, bufs.neighbor, bufs.add, bufs.remove, bufs.positives_remove, stats[3])
    s = stats.cpu().numpy()
    for step in range(3):
        sc = b._scalars(s[step])
        got = (sc['loss'], sc['add_prc'], sc['add_rcl'], sc['remove_prc'], sc['remove_rcl'])
        assert [float(x).hex() for x in got] == [float(x).hex() for x in host_scalars[step]], step
    ev = b._scalars(s[3])
    assert sorted(ev) == sorted(host_eval) and all(float(ev[k]).hex() == float(host_eval[k]).hex() for k in ev)
    wa, wb = a.weights_numpy(), b.weights_numpy()
    assert a.step == b.step == 3
    for k in wa:
        assert wa[k].tobytes() == wb[k].tobytes(), k
    for sa, sb in zip(a.slots_numpy(), b.slots_numpy()):
        for k in sa:
            assert sa[k].tobytes() == sb[k].tobytes(), k
    with pytest.raises(ValueError):
        b.train_step_device(bufs.inlier, bufs.neighbor, bufs.add, bufs.remove, bufs.positives_remove.to(torch.int64), stats[0])


# ---------------------------------------------------------------- 4. staging left on the device ----------------------------------------------------------------
def test_staging_left_on_the_device_holds_the_downloaded_rows(cuda_device):
    rooms = stage_ref.gpu_rooms()[:3]                                          # the second is the one-point room that emits nothing
    info_down, info_left = {}, {}
    down = stage.stage_rooms_gpu(rooms, seed=stage_ref.RNG_SEED, device=cuda_device, info=info_down)
    left = stage.stage_rooms_gpu(rooms, seed=stage_ref.RNG_SEED, device=cuda_device, info=info_left, download=False)
    dev = left['device']
    assert left['points'] == [] and left['neighbor_points'] == [] and len(down['points']) > 100
    for key in ('points', 'remove', 'neighbor_points', 'add'):
        want = np.concatenate(down[key])
        got = dev[key].cpu().numpy()
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), key
    assert dev['row_in'].tolist() == np.concatenate([[0], np.cumsum([len(p) for p in down['points']])]).tolist()
    assert dev['row_nb'].tolist() == np.concatenate([[0], np.cumsum([len(p) for p in down['neighbor_points']])]).tolist()
    assert left['steps'] == down['steps'] and np.array_equal(np.array(left['complete'], np.float32), np.array(down['complete'], np.float32))
    assert info_left['tuples'] == info_down['tuples'] and 0 < info_left['bytes_downloaded'] < info_down['bytes_downloaded']
    rows_bytes = sum(dev[key].numel() * dev[key].element_size() for key in ('points', 'remove', 'neighbor_points', 'add'))
    assert info_down['bytes_downloaded'] - info_left['bytes_downloaded'] == rows_bytes
    # the store over the device buffers and the store over the downloaded tuples draw the same batch
    a = TupleStore.from_device(dev, 13, rng_seed=2)
    keep = [i for i in range(len(down['points'])) if len(down['neighbor_points'][i]) > 0]
    b = TupleStore.from_staged({k: [down[k][i] for i in keep] for k in ('points', 'remove', 'neighbor_points', 'add')}, 13, cuda_device, rng_seed=2)
    assert len(a) == len(b) == len(keep)
    both = TupleStore.concat([a, b])
    assert len(both) == 2 * len(a)
    order = [0, len(a) - 1, len(a) // 2]
    bufs = [BatchBuffers(3, K, K, 13, cuda_device) for _ in range(3)]
    a.assemble(a.upload_order(order), 1, 0, bufs[0])
    b.assemble(b.upload_order(order), 1, 0, bufs[1])
    both.assemble(both.upload_order(order), 1, 0, bufs[2])                     # ids below len(a): the same tuples under the same ids
    for name in ('inlier', 'neighbor', 'add', 'remove', 'positives_remove', 'positives_add'):
        x = getattr(bufs[0], name).cpu().numpy().tobytes()
        assert x == getattr(bufs[1], name).cpu().numpy().tobytes() == getattr(bufs[2], name).cpu().numpy().tobytes(), name


# ---------------------------------------------------------------- 5. the driver ----------------------------------------------------------------
def test_driver_from_staged_file_and_online_agree(cuda_device, tmp_path, capsys):
    """stage_data.py --rng counter writes a file; one epoch from that file with --assemble device and one epoch staged online from the room
    file draw the same batches: the same Epoch line, the same checkpoint bytes."""
    import stage_data
    import train_region_grow
    from learn_region_grow_amd import io as lio
    raw = [synthetic.area5_shaped_room(600, seed=5).astype(np.float32), synthetic.area5_shaped_room(500, seed=6).astype(np.float32)]
    lio.saveToH5(str(tmp_path / 'synthetic_unit.h5'), raw)
    stage_data.main(['--area', 'synthetic_unit', '--data-dir', str(tmp_path), '--rng', 'counter', '--max-points', '512', '--quiet'])
    staged = str(tmp_path / 'staged_synthetic_unit.h5')
    capsys.readouterr()

    def epoch_lines(argv):
        assert train_region_grow.main(argv) == 0
        return [x for x in capsys.readouterr().out.splitlines() if x.startswith('Epoch ')]
    common = ['--epochs', '1', '--batch-size', '4', '--seed', '3']
    ck_a, ck_b, ck_c = (str(tmp_path / d / 'lrgnet_unit.ckpt') for d in ('a', 'b', 'c'))
    line_a = epoch_lines(['--staged', staged, '--assemble', 'device', '--multiseed', '0', '--ckpt', ck_a] + common)
    online = ['--stage', 'online', '--train-area', 'synthetic_unit', '--data-dir', str(tmp_path), '--max-points', '512']
    line_b = epoch_lines(online + ['--multiseed', '1', '--ckpt', ck_b] + common)
    assert len(line_a) == 1 and line_a[0].startswith('Epoch 0 loss ') and np.isfinite(float(line_a[0].split()[3]))
    assert line_a == line_b
    files_a, files_b = sorted(glob.glob(ck_a + '*')), sorted(glob.glob(ck_b + '*'))
    data_a = [f for f in files_a if '.data-' in f]
    assert data_a and [os.path.basename(f) for f in files_a] == [os.path.basename(f) for f in files_b]
    for fa, fb in zip(files_a, files_b):
        if '.data-' in fa:
            assert open(fa, 'rb').read() == open(fb, 'rb').read(), os.path.basename(fa)
    lines = epoch_lines(online + ['--multiseed', '2', '--ckpt', ck_c, '--epochs', '2', '--batch-size', '4', '--seed', '3'])
    assert [x.split()[1] for x in lines] == ['0', '1']
    for x in lines:
        assert all(np.isfinite(float(v)) for v in (x.split()[3],) + tuple(x.split()[5].split('/')) + tuple(x.split()[7].split('/')))
    assert lines[0] == line_a[0]                                               # seed 0 of two is the unseeded staging again
