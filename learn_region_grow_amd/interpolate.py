"""tf_ops/3d_interpolation replacements on torch tensors (HIP kernels through the C-ABI; the reference runs these on the CPU).

Same names and argument order as the reference's Python wrappers (tf_ops/3d_interpolation/tf_interpolate.py:8,19,30):
``three_nn(xyz1, xyz2)``, ``three_interpolate(points, idx, weight)`` and ``three_interpolate_grad(points, idx, weight, grad_out)``
(the registered gradient), plus ``three_nn_interpolate``: the interpolation of pointnet_fp_module (train_pointnet.py:145-150)
in one launch.  Shape errors raise ``ValueError`` where the reference op raises ``InvalidArgument`` (tf_interpolate.cpp:163-243).
"""
import torch

from . import _lib
from .grouping import _chk
from .lrgnet import _ptr, _stream_ptr


def _chk_xyz(xyz1, xyz2):
    xyz1 = _chk(xyz1, 3, torch.float32, 'xyz1')
    xyz2 = _chk(xyz2, 3, torch.float32, 'xyz2')
    if xyz1.shape[2] != 3:
        raise ValueError('ThreeNN expects (b,n,3) xyz1 shape.')
    if xyz2.shape[2] != 3 or xyz2.shape[0] != xyz1.shape[0]:
        raise ValueError('ThreeNN expects (b,m,3) xyz2 shape.')
    return xyz1, xyz2


def three_nn(xyz1, xyz2):
    """xyz1 (b,n,3) unknown points, xyz2 (b,m,3) known points -> dist (b,n,3) SQUARED distances, idx (b,n,3) int32."""
    xyz1, xyz2 = _chk_xyz(xyz1, xyz2)
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    dist = torch.empty((b, n, 3), dtype=torch.float32, device=xyz1.device)
    idx = torch.empty((b, n, 3), dtype=torch.int32, device=xyz1.device)
    _lib.check(_lib.load().lrg_three_nn(b, n, m, _ptr(xyz1), _ptr(xyz2), _ptr(dist), _ptr(idx), _stream_ptr()), 'lrg_three_nn')
    return dist, idx


def _chk_interp(points, idx, weight):
    points = _chk(points, 3, torch.float32, 'points')
    idx = _chk(idx, 3, torch.int32, 'idx')
    weight = _chk(weight, 3, torch.float32, 'weight')
    b = points.shape[0]
    if idx.shape[0] != b or idx.shape[2] != 3:
        raise ValueError('ThreeInterpolate expects (b,n,3) idx shape')
    if tuple(weight.shape) != (b, idx.shape[1], 3):
        raise ValueError('ThreeInterpolate expects (b,n,3) weight shape')
    return points, idx, weight


def three_interpolate(points, idx, weight):
    """points (b,m,c), idx (b,n,3) int32, weight (b,n,3) -> (b,n,c)."""
    points, idx, weight = _chk_interp(points, idx, weight)
    b, m, c = points.shape
    n = idx.shape[1]
    out = torch.empty((b, n, c), dtype=torch.float32, device=points.device)
    _lib.check(_lib.load().lrg_three_interpolate(b, m, c, n, _ptr(points), _ptr(idx), _ptr(weight), _ptr(out), _stream_ptr()),
               'lrg_three_interpolate')
    return out


def three_interpolate_grad(points, idx, weight, grad_out):
    """Gradient of three_interpolate w.r.t. points: grad_out (b,n,c) -> (b,m,c), scattered with atomics."""
    points, idx, weight = _chk_interp(points, idx, weight)
    grad_out = _chk(grad_out, 3, torch.float32, 'grad_out')
    b, m, c = points.shape
    n = idx.shape[1]
    if tuple(grad_out.shape) != (b, n, c):
        raise ValueError('ThreeInterpolateGrad expects (b,n,c) grad_out shape')
    gp = torch.zeros((b, m, c), dtype=torch.float32, device=points.device)
    _lib.check(_lib.load().lrg_three_interpolate_grad(b, n, c, m, _ptr(grad_out), _ptr(idx), _ptr(weight), _ptr(gp), _stream_ptr()),
               'lrg_three_interpolate_grad')
    return gp


def three_nn_interpolate(xyz1, xyz2, points2, return_weight=False):
    """three_nn, the inverse-distance weights of pointnet_fp_module (1/max(d, 1e-10), normalised) and three_interpolate in one
    launch: xyz1 (b,n,3), xyz2 (b,m,3) with m >= 1, points2 (b,m,c) -> (b,n,c); with return_weight also the weights (b,n,3)."""
    xyz1, xyz2 = _chk_xyz(xyz1, xyz2)
    points2 = _chk(points2, 3, torch.float32, 'points2')
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    if points2.shape[0] != b or points2.shape[1] != m:
        raise ValueError('ThreeInterpolate expects (b,m,c) points shape')
    if m == 0:
        raise ValueError('three_nn_interpolate needs at least one known point')
    c = points2.shape[2]
    out = torch.empty((b, n, c), dtype=torch.float32, device=xyz1.device)
    weight = torch.empty((b, n, 3), dtype=torch.float32, device=xyz1.device) if return_weight else None
    _lib.check(_lib.load().lrg_three_nn_interpolate(b, n, m, c, _ptr(xyz1), _ptr(xyz2), _ptr(points2), None, None, _ptr(weight),
                                                    _ptr(out), _stream_ptr()), 'lrg_three_nn_interpolate')
    return (out, weight) if return_weight else out
