"""tf_ops/sampling replacements on torch tensors (HIP kernels through the C-ABI).

Same names and argument order as the reference's Python wrappers (tf_ops/sampling/tf_sampling.py:13,29,44,48):
``prob_sample(inp, inpr)``, ``gather_point(inp, idx)``, ``gather_point_grad(inp, idx, out_g)`` (the registered gradient)
and ``farthest_point_sample(npoint, inp)``.  Shape errors raise ``ValueError`` where the reference op raises
``InvalidArgument`` (tf_sampling.cpp:76-79,99,105,131-135,156-167).
"""
import torch

from . import _lib
from .grouping import _chk
from .lrgnet import _ptr, _stream_ptr

FPS_REGISTER_POINTS = 16384      # lrg_farthest_point_sample: up to this many points per batch element need no workspace


def prob_sample(inp, inpr):
    """inp (b,ncategory) non-negative weights, inpr (b,npoints) uniform in [0,1) -> (b,npoints) int32 category indices."""
    inp = _chk(inp, 2, torch.float32, 'inp')
    inpr = _chk(inpr, 2, torch.float32, 'inpr')
    if inpr.shape[0] != inp.shape[0]:
        raise ValueError('ProbSample expects (batch_size,num_points) inpr shape')
    b, n = inp.shape
    m = inpr.shape[1]
    if n == 0 and b * m > 0:
        raise ValueError('ProbSample expects at least one category')
    out = torch.empty((b, m), dtype=torch.int32, device=inp.device)
    temp = torch.empty((b, n), dtype=torch.float32, device=inp.device)
    _lib.check(_lib.load().lrg_prob_sample(b, n, m, _ptr(inp), _ptr(inpr), _ptr(temp), _ptr(out), _stream_ptr()), 'lrg_prob_sample')
    return out


def gather_point(inp, idx):
    """inp (b,ndataset,3), idx (b,npoints) int32 -> (b,npoints,3)."""
    inp = _chk(inp, 3, torch.float32, 'inp')
    idx = _chk(idx, 2, torch.int32, 'idx')
    if inp.shape[2] != 3:
        raise ValueError('GatherPoint expects (batch_size,num_points,3) inp shape')
    if idx.shape[0] != inp.shape[0]:
        raise ValueError('GatherPoint expects (batch_size,num_result) idx shape')
    b, n, _ = inp.shape
    m = idx.shape[1]
    out = torch.empty((b, m, 3), dtype=torch.float32, device=inp.device)
    _lib.check(_lib.load().lrg_gather_point(b, n, m, _ptr(inp), _ptr(idx), _ptr(out), _stream_ptr()), 'lrg_gather_point')
    return out


def gather_point_grad(inp, idx, out_g):
    """Gradient of gather_point w.r.t. inp: scatter-add of out_g (b,npoints,3) into (b,ndataset,3)."""
    inp = _chk(inp, 3, torch.float32, 'inp')
    idx = _chk(idx, 2, torch.int32, 'idx')
    out_g = _chk(out_g, 3, torch.float32, 'out_g')
    if inp.shape[2] != 3:
        raise ValueError('GatherPointGradGpuOp expects (batch_size,num_points,3) inp')
    b, n, _ = inp.shape
    if idx.shape[0] != b:
        raise ValueError('GatherPointGradGpuOp expects (batch_size,num_result) idx shape')
    m = idx.shape[1]
    if tuple(out_g.shape) != (b, m, 3):
        raise ValueError('GatherPointGradGpuOp expects (batch_size,num_result,3) out_g shape')
    inp_g = torch.zeros((b, n, 3), dtype=torch.float32, device=inp.device)
    _lib.check(_lib.load().lrg_scatter_add_point(b, n, m, _ptr(out_g), _ptr(idx), _ptr(inp_g), _stream_ptr()), 'lrg_scatter_add_point')
    return inp_g


def farthest_point_sample(npoint, inp):
    """npoint > 0, inp (b,ndataset,3) -> (b,npoint) int32, the reference's indices including its choice among ties
    (include/lrg_hip.h: lrg_farthest_point_sample)."""
    if npoint <= 0:
        raise ValueError('FarthestPointSample expects positive npoint')
    inp = _chk(inp, 3, torch.float32, 'inp')
    if inp.shape[2] != 3:
        raise ValueError('FarthestPointSample expects (batch_size,num_points,3) inp shape')
    b, n, _ = inp.shape
    if n == 0 and b > 0:
        raise ValueError('FarthestPointSample expects at least one point')
    out = torch.empty((b, npoint), dtype=torch.int32, device=inp.device)
    temp = torch.empty((b, n), dtype=torch.float32, device=inp.device) if n > FPS_REGISTER_POINTS else None
    _lib.check(_lib.load().lrg_farthest_point_sample(b, n, npoint, _ptr(inp), _ptr(temp), _ptr(out), _stream_ptr()),
               'lrg_farthest_point_sample')
    return out
