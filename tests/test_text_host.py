"""CPU: the integer algorithm behind lrg_text_encode equals Python's '%f' (tests/text_ref.py, the twin the kernel is read against), the
longest line fits LRG_TEXT_MAX_LINE, and the kernel's own arithmetic header, compiled for the host, agrees with printf."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import text_ref
from conftest import REPO

PICKED = [0.0, -0.0, 1e-9, -1e-9, 5e-7, float(np.nextafter(np.float32(5e-7), np.float32(0))), float(np.nextafter(np.float32(5e-7), np.float32(1))),
          4.9999997e-7, 0.9999995, 9.9999995, 999999.97, 1e-45, -1e-45, 123456.789, 2.0 ** 39, -2.0 ** 39, 0.0078125, -0.0078125, 0.0234375,
          2.0 ** 40 - 2.0 ** 16, 1.17549435e-38, 1e-40]


def _values():
    rs = np.random.RandomState(7)
    normals = (rs.randn(60000) * 8).astype(np.float32)
    ties = (np.arange(-(1 << 20), (1 << 20) + 1, dtype=np.int64) / 128.0).astype(np.float32)      # every multiple of 1/128 in +-2^13
    bits = (rs.randint(0, 1 << 23, 60000).astype(np.uint32) | (rs.randint(0, text_ref.LIMIT_EXPONENT, 60000).astype(np.uint32) << 23) |
            (rs.randint(0, 2, 60000).astype(np.uint32) << 31))
    return np.concatenate([normals, ties, bits.view(np.float32), np.array(PICKED, dtype=np.float32)])


def test_twin_equals_python_percent_f():
    v = _values()
    assert len(v) >= 200000
    got = text_ref.format_many(v)
    want = ['%f' % x for x in v.tolist()]                    # tolist(): the float32 value widened to a Python float, as savePLY's p[0] prints
    wrong = [(float(x), g, w) for x, g, w in zip(v, got, want) if g != w]
    assert not wrong, wrong[:10]
    for x in PICKED:                                          # ... and the scalar twin on the hand-picked values
        assert text_ref.format_f(np.float32(x)) == '%f' % float(np.float32(x)), x
    assert text_ref.format_f(np.float32(0.0078125)) == '0.007812' and text_ref.format_f(np.float32(0.0234375)) == '0.023438'      # ties go to even
    assert text_ref.format_f(np.float32(-0.0)) == '-0.000000' and text_ref.format_f(np.float32(-1e-9)) == '-0.000000'
    assert text_ref.format_f(np.float32(0.9999995)) == '1.000000'


def test_refused_values():
    for x in (np.inf, -np.inf, np.nan, 2.0 ** 40, -2.0 ** 40, 3e38):
        assert text_ref.format_f(np.float32(x)) is None
    assert text_ref.format_f(np.float32(2.0 ** 40 - 2.0 ** 16)) == '%f' % (2.0 ** 40 - 2.0 ** 16)
    assert text_ref.line([0, 0, 0], [0, 0, 256], 'pcd') is None and text_ref.line([0, 0, 0], [-1, 0, 0], 'pcd') is None
    assert text_ref.line([0, 0, 0], [0, 0, 256], 'ply') == '0.000000 0.000000 0.000000 0 0 256\n'


def test_longest_line_fits():
    from learn_region_grow_amd import _lib
    x = -(2.0 ** 40 - 2.0 ** 16)
    ln = text_ref.line([x, x, x], [-2 ** 31] * 3)
    assert ln == '%f %f %f %d %d %d\n' % (x, x, x, -2 ** 31, -2 ** 31, -2 ** 31)
    assert len(ln) == text_ref.LRG_TEXT_MAX_LINE == _lib.LRG_TEXT_MAX_LINE == 102
    assert len(text_ref.line([x, x, x], [255, 255, 255], 'pcd')) <= _lib.LRG_TEXT_MAX_LINE


def test_kernel_arithmetic_on_the_host(tmp_path):
    """csrc/lrg_text_fmt.h -- the code both passes of the kernel run -- compiled for the host against printf (tools/text_fmt_check.cpp)."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler to build tools/text_fmt_check.cpp with')
    exe = str(tmp_path / 'text_fmt_check')
    subprocess.check_call([cxx, '-std=c++17', '-O2', os.path.join(REPO, 'tools', 'text_fmt_check.cpp'), '-o', exe])
    r = subprocess.run([exe, '50000'], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith('ok '), r.stdout[-2000:]
