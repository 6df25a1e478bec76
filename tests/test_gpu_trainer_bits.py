"""GPU: the PointNet and PointNet2 trainers give, bit for bit, what tests/golden/trainer_bits.json records.

Both trainers add in a fixed order (no float atomic anywhere), so a change that only moves code leaves every bit where it was.  Per
case: init_weights(seed) -- the order of the generator's draws is part of the record -- three train_steps on seeded, slightly
perturbed points, one evaluate on a batch of another cell count; recorded are the SHA-256 of the bytes of flat, m, v, gflat (and
ema), the SHA-256 of checkpoint_numpy()'s sorted keys and bytes, and float.hex of every returned loss and accuracy.

A change that means to alter the arithmetic records the file again on the GPU, with

    python tests/test_gpu_trainer_bits.py --record --commit <the commit recorded from>

and says so; the file's "recorded" field names the commit and the command that wrote it.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from trainer_helpers import P, f32, three_cells      # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN_FILE = os.path.join(GOLDEN, 'trainer_bits.json')
RECORD_COMMAND = 'python tests/test_gpu_trainer_bits.py --record'

# PointNet: (conv widths or the name of an architecture, fc widths, classes, B, trainer options); PointNet2: (classes, rgb, B)
CASES = {'pointnet-tiny': ('pointnet', (32, 32), (32,), 3, 3, {}),              # nc == 2: the skip's gradient joins in head_input_backward
         'pointnet-shipped': ('pointnet', 'shipped', None, 13, 2, {}),
         'pointnet-today': ('pointnet', 'today', None, 13, 2, dict(decay_steps=2)),      # two batch-norm blocks; the rate halves inside the run
         'pointnet2-rgb': ('pointnet2', 13, True, 3),
         'pointnet2-xyz': ('pointnet2', 260, False, 1)}                         # the single-cell colsum plan


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def build(name, device):
    """(trainer, training points [B,1024,6], labels, evaluation points of another cell count, their labels)."""
    case = CASES[name]
    seed = sorted(CASES).index(name)
    rs = np.random.RandomState(100 + seed)
    if case[0] == 'pointnet':
        from learn_region_grow_amd.pointnet_train import ARCHITECTURES, PointNetTrainer
        _, conv, fc, ncls, B, kw = case
        if isinstance(conv, str):
            conv, fc = ARCHITECTURES[conv]
        tr = PointNetTrainer(B, conv, fc, ncls, device=device, **kw)
        cells = rs.uniform(-1, 1, (B + 3, P, 6)).astype(f32)
        cells[:, :, 2] = rs.uniform(0, 2.5, (B + 3, P))
    else:
        from learn_region_grow_amd.pointnet2_train import PointNet2Trainer
        _, ncls, rgb, B = case
        tr = PointNet2Trainer(B, ncls, rgb, device=device)
        cells = np.concatenate([three_cells(200 + seed), three_cells(300 + seed)])
    n_eval = 3 if B == 2 else 2
    lab = rs.randint(0, ncls, (len(cells), P))
    tr.init_weights(7 + seed)
    return tr, cells[:B], lab[:B], cells[-n_eval:], lab[-n_eval:]


def run_case(name, device):
    """name of a recorded quantity -> its digest (or list of float.hex), in the order the test compares them."""
    tr, pts, lab, eval_pts, eval_lab = build(name, device)
    rs = np.random.RandomState(3)
    scalars = []
    for _ in range(3):
        sc = tr.train_step(pts + rs.uniform(-0.01, 0.01, pts.shape).astype(f32), lab)
        scalars += [float(sc['loss']).hex(), float(sc['acc']).hex()]
    ev = tr.evaluate(eval_pts, eval_lab)
    scalars += [float(ev['loss']).hex(), float(ev['acc']).hex()]
    out = {'scalars': scalars}
    for buf in ('flat', 'm', 'v', 'gflat', 'ema'):
        if hasattr(tr, buf):
            out[buf] = sha(getattr(tr, buf).cpu().numpy())
    ck = tr.checkpoint_numpy()
    h = hashlib.sha256()
    for k in sorted(ck):
        h.update(k.encode('utf-8'))
        h.update(np.ascontiguousarray(ck[k]).tobytes())
    out['checkpoint'] = h.hexdigest()
    return out


@pytest.mark.parametrize('name', sorted(CASES))
def test_trainer_bits_are_the_recorded_ones(cuda_device, name):
    with open(GOLDEN_FILE) as f:
        want = json.load(f)['cases'][name]
    got = run_case(name, cuda_device)
    assert sorted(got) == sorted(want)
    for key in ('scalars', 'gflat', 'flat', 'm', 'v', 'ema', 'checkpoint'):
        if key in want:
            assert got[key] == want[key], '%s: %s is the first that differs from %s' % (name, key, os.path.basename(GOLDEN_FILE))


def record(argv):
    import argparse
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--record', action='store_true', required=True)
    ap.add_argument('--commit', default='unknown', help='the commit whose trainers are recorded')
    ap.add_argument('--out', default=GOLDEN_FILE)
    a = ap.parse_args(argv)
    device = torch.device('cuda:0')
    cases = {name: run_case(name, device) for name in sorted(CASES)}
    doc = dict(recorded=dict(commit=a.commit, command=RECORD_COMMAND + ' --commit ' + a.commit,
                             how='run the command on an MI355X from a tree whose trainers are that commit\'s; a change that means to '
                                 'alter the arithmetic records again and says so'),
               cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(cases, sort_keys=True))


if __name__ == '__main__':
    record(sys.argv[1:])
