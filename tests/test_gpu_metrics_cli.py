"""GPU: --metrics device of the command lines -- the evaluation of all rooms in one device pass feeds the same room lines, aggregate line
and --save colouring as --metrics host (the default)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from learn_region_grow_amd import checkpoint, synthetic
from learn_region_grow_amd import io as lio

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp('metrics_cli')
    raw = [synthetic.generate_room_points(700 + 60 * i, 90 + i, wlh=(1.2 + 0.15 * i, 1.1, 1.0)).astype(np.float32) for i in range(2)]
    h5 = str(d / 'rooms.h5')
    lio.saveToH5(h5, raw)
    weights = synthetic.make_synthetic_weights(seed=0, gain=2.0, bias_std=0.2, add_bias_shift=0.0, rmv_bias_shift=-3.0)
    prefix = str(d / 'lrgnet.ckpt')
    checkpoint.write_bundle(prefix, weights)
    return d, h5, prefix


def _run(script, args, cwd):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, capture_output=True, text=True, cwd=str(cwd), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


def _metric_lines(lines):
    got = [ln for ln in lines if ln.startswith(('Area ', 'NMI: '))]
    assert len(got) == 3 and got[-1].startswith('NMI: ')
    return got


def test_region_grow_device_metrics_print_and_save_the_same(cuda_device, inputs):
    d, h5, prefix = inputs
    base = ['--h5', h5, '--ckpt', prefix, '--policy', 'gt', '--seed', '6', '--quiet-regions']
    host = _run('region_grow.py', base + ['--save', str(d / 'host')], d)
    dev = _run('region_grow.py', base + ['--save', str(d / 'device'), '--metrics', 'device'], d)
    assert _metric_lines(dev) == _metric_lines(host)
    for i in range(2):
        a, b = open(d / 'host' / ('%d.ply' % i), 'rb').read(), open(d / 'device' / ('%d.ply' % i), 'rb').read()
        assert len(a) > 1000 and a == b


def test_baselines_device_metrics_print_the_same(cuda_device, inputs):
    d, h5, _ = inputs
    base = ['--h5', h5, '--area', '5', '--mode', 'color']
    assert _metric_lines(_run('baselines.py', base + ['--metrics', 'device'], d)) == _metric_lines(_run('baselines.py', base, d))


def test_mcpnet_device_metrics_print_and_save_the_same(cuda_device, tmp_path):
    """order='set' through the command line: the golden rooms and weights of tests/test_gpu_mcpnet.py."""
    import mcpnet_ref
    from conftest import GOLDEN
    golden = np.load(os.path.join(GOLDEN, 'mcpnet_ref_cpu.npz'))
    z = np.load(os.path.join(GOLDEN, 'mcpnet_model5_weights.npz'))
    h5, ck = str(tmp_path / 'rooms.h5'), str(tmp_path / 'm' / 'mcp.ckpt')
    lio.saveToH5(h5, mcpnet_ref.golden_rooms(tuple(int(s) for s in golden['seeds'])))
    checkpoint.write_bundle(ck, {k: z[k] for k in z.files})
    base = ['--h5', h5, '--area', '5', '--ckpt', ck]
    host = _run('mcpnet.py', base + ['--save', str(tmp_path / 'host')], tmp_path)
    dev = _run('mcpnet.py', base + ['--save', str(tmp_path / 'device'), '--metrics', 'device'], tmp_path)
    got, want = [ln for ln in dev if ln.startswith(('Area ', 'NMI: '))], [ln for ln in host if ln.startswith(('Area ', 'NMI: '))]
    assert len(want) >= 3 and got == want
    assert want[:-1] == [str(x) for x in golden['room_lines']]
    for i in range(len(want) - 1):
        a, b = open(tmp_path / 'host' / 'results' / ('%d.ply' % i), 'rb').read(), open(tmp_path / 'device' / 'results' / ('%d.ply' % i), 'rb').read()
        assert len(a) > 1000 and a == b
