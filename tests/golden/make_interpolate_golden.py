#!/usr/bin/env python3
"""Generate tests/golden/interpolate_ref_cpu.npz from the REFERENCE's own CPU functions (golden-making time only).

    python tests/golden/make_interpolate_golden.py <reference checkout>

threenn_cpu, threeinterpolate_cpu and threeinterpolate_grad_cpu are cut out of
<reference>/tf_ops/3d_interpolation/tf_interpolate.cpp into a temporary directory, compiled there with g++ (no FMA) into a
shared library, and run on fixed inputs.  Only the inputs and outputs are saved; no reference source is kept.  Cases cover
equal distances (integer grids), duplicate known points, m = 1 and m = 2 (missing neighbours), random data, and
integer-valued gradient inputs (exact in any summation order)."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32


def _build(ref, tmp):
    src = open(os.path.join(ref, 'tf_ops', '3d_interpolation', 'tf_interpolate.cpp')).read()
    start = src.index('void threenn_cpu')
    end = src.index('class ThreeNNOp')
    body = src[start:end]
    for name in ('threenn_cpu', 'threeinterpolate_cpu', 'threeinterpolate_grad_cpu'):
        assert re.search(r'void %s\(' % name, body), name
    cpp = os.path.join(tmp, 'interp.cpp')
    with open(cpp, 'w') as f:
        f.write('extern "C" {\n' + body + '\n}\n')
    so = os.path.join(tmp, 'libinterp.so')
    subprocess.check_call(['g++', '-O2', '-fPIC', '-shared', '-ffp-contract=off', '-fno-fast-math', '-o', so, cpp])
    lib = ctypes.CDLL(so)
    for fn in (lib.threenn_cpu, lib.threeinterpolate_cpu, lib.threeinterpolate_grad_cpu):
        fn.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run_cases(lib):
    rs = np.random.RandomState(20261015)
    cases = {}

    def add(name, xyz1, xyz2, c, integer_values):
        xyz1 = np.ascontiguousarray(xyz1, F32)
        xyz2 = np.ascontiguousarray(xyz2, F32)
        b, n, _ = xyz1.shape
        m = xyz2.shape[1]
        dist = np.zeros((b, n, 3), F32)
        idx = np.zeros((b, n, 3), np.int32)
        lib.threenn_cpu(b, n, m, _p(xyz1), _p(xyz2), _p(dist), _p(idx))
        if integer_values:
            points = rs.randint(-8, 9, size=(b, m, c)).astype(F32)
            weight = rs.randint(-3, 4, size=(b, n, 3)).astype(F32)
            grad_out = rs.randint(-8, 9, size=(b, n, c)).astype(F32)
        else:
            points = rs.randn(b, m, c).astype(F32)
            weight = rs.rand(b, n, 3).astype(F32)
            grad_out = rs.randn(b, n, c).astype(F32)
        out = np.zeros((b, n, c), F32)
        lib.threeinterpolate_cpu(b, m, c, n, _p(points), _p(idx), _p(weight), _p(out))
        grad_points = np.zeros((b, m, c), F32)
        lib.threeinterpolate_grad_cpu(b, n, c, m, _p(grad_out), _p(idx), _p(weight), _p(grad_points))
        for k, v in dict(xyz1=xyz1, xyz2=xyz2, dist=dist, idx=idx, points=points, weight=weight, out=out, grad_out=grad_out,
                         grad_points=grad_points).items():
            cases['%s__%s' % (name, k)] = v

    add('random', rs.rand(2, 300, 3), rs.rand(2, 70, 3), 8, False)
    grid = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(2), indexing='ij'), -1).reshape(1, -1, 3).astype(F32)
    add('grid_ties', rs.randint(0, 4, size=(2, 64, 3)) + 0.5 * rs.randint(0, 2, size=(2, 64, 3)), np.repeat(grid, 2, 0), 5, True)
    dup = rs.randint(0, 3, size=(1, 6, 3)).astype(F32)
    add('duplicates', rs.randint(0, 3, size=(1, 40, 3)), np.concatenate([dup, dup, dup[:, :2]], 1), 4, True)
    add('m1', rs.rand(2, 17, 3), rs.rand(2, 1, 3), 3, True)
    add('m2', rs.rand(2, 17, 3), rs.rand(2, 2, 3), 3, True)
    add('random_int', rs.rand(3, 129, 3), rs.rand(3, 33, 3), 16, True)
    return cases


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        cases = run_cases(_build(sys.argv[1], tmp))
    path = os.path.join(HERE, 'interpolate_ref_cpu.npz')
    np.savez_compressed(path, **cases)
    print('wrote', path, len(cases), 'arrays')


if __name__ == '__main__':
    main()
