"""GPU: --ply-encoder device of the command lines writes the files --ply-encoder host (the default) writes, byte for byte, and prints the
same lines."""
import os
import subprocess
import sys

import numpy as np
import pytest

from learn_region_grow_amd import io as lio
from learn_region_grow_amd import synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def rooms(tmp_path_factory):
    d = tmp_path_factory.mktemp('ply_encoder_cli')
    raw = [synthetic.generate_room_points(900 + 250 * i, 70 + i, wlh=(1.2 + 0.15 * i, 1.1, 1.0)).astype(np.float32) for i in range(2)]
    h5 = str(d / 'rooms.h5')
    lio.saveToH5(h5, raw)
    return d, h5, [len(r) for r in raw]


def _run(script, args, cwd):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, capture_output=True, text=True, cwd=str(cwd), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def _same(d, script, base, timed, sizes):
    """The two runs' stdout without the one kind of line that carries a measured time (`timed`), and their files."""
    outs = {}
    for how in ('host', 'device'):
        (d / how).mkdir(parents=True)
        out = _run(script, base + ['--save', 'ply', '--ply-encoder', how], d / how)
        outs[how] = [ln for ln in out.splitlines() if timed not in ln]
        assert len(outs[how]) < len(out.splitlines())
    assert outs['device'] == outs['host']
    assert [ln for ln in outs['device'] if ln.startswith('Saved to ply/')] == ['Saved to ply/%d.ply: (%d points)' % (i, n) for i, n in enumerate(sizes)]
    for i in range(2):
        a, b = open(d / 'host' / 'ply' / ('%d.ply' % i), 'rb').read(), open(d / 'device' / 'ply' / ('%d.ply' % i), 'rb').read()
        assert len(a) > 1000 and a == b


def test_region_grow_ply_encoder(cuda_device, rooms):
    d, h5, sizes = rooms
    # (the summary line, '2 rooms on 1 GPU(s): preprocessing 0.31 s ...', carries measured times: left out of the comparison)
    _same(d / 'lrg', 'region_grow.py', ['--h5', h5, '--synthetic-weights', '--policy', 'gt', '--seed', '6', '--quiet-regions'], ' GPU(s): preprocessing ', sizes)


def test_baselines_ply_encoder(cuda_device, rooms):
    d, h5, sizes = rooms
    # (the room's timing line, '<name> <n> points: 0.12s', carries a measured time: left out of the comparison)
    _same(d / 'normal', 'baselines.py', ['--h5', h5, '--area', '5', '--mode', 'normal'], ' points: ', sizes)
