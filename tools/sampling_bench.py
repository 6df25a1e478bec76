#!/usr/bin/env python3
"""tf_ops/sampling and tf_ops/3d_interpolation replacements at the PointNet2 shapes (train_pointnet.py:180-190, b = 100, n = 1024):
    FPS 1024 -> 1024, 1024 -> 256, 256 -> 64, 64 -> 16 (the set-abstraction levels; 1024 -> 1024 is the first level's npoint = n)
    three_nn / three_interpolate / the fused three_nn_interpolate for the feature-propagation levels 64 <- 16 (c = 512),
    256 <- 64, 1024 <- 256 and 1024 <- 1024 (c = 128)
    scene-size FPS: n = 32 768 and 131 072, m = 1024, b = 1 (one workgroup: the streaming path)
GPU: HIP events round `reps` (>= 100) back-to-back launches of the C entry points on preallocated buffers.
Rooflines:
  - FPS is a chain of m - 1 dependent steps (each a full argmax over the batch element's points): reported as us per step;
  - three_nn is priced by its n x m distance evaluations; one evaluation (3 sub, 3 mul, 2 add, the cascade's compare) counted as 9
    vector fp32 operations against 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 39.3 T ops/s;
  - gather_point, three_interpolate (and the fused op's interpolation) by the bytes that must reach HBM (inputs once, outputs)
    against 8 TB/s.
Prints one JSON object (also importable: sampling_rates())."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM = 8000e9
VALU = 256 * 4 * 16 * 2.4e9
NN_OPS = 9


def _time_gpu(fn, reps=100):
    import torch
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def sampling_rates(device='cuda:0', reps=100):
    import torch
    from learn_region_grow_amd import _lib
    from learn_region_grow_amd.lrgnet import _ptr, _stream_ptr
    lib = _lib.load()
    dev = torch.device(device)
    g = torch.Generator(device='cpu').manual_seed(0)
    out = {}

    def fps_row(b, n, m, r):
        x = torch.rand((b, n, 3), generator=g).to(dev)
        o = torch.empty((b, m), dtype=torch.int32, device=dev)
        tmp = torch.empty((b, n), device=dev) if n > 16384 else None

        def f():
            _lib.check(lib.lrg_farthest_point_sample(b, n, m, _ptr(x), _ptr(tmp), _ptr(o), _stream_ptr()), 'fps')
        t = _time_gpu(f, r)
        return dict(b=b, n=n, m=m, gpu_us=t * 1e6, us_per_step=t * 1e6 / max(1, m - 1),
                    path='registers' if n <= 16384 else 'streaming (temp in HBM / L2)')
    for n, m in ((1024, 1024), (1024, 256), (256, 64), (64, 16)):
        out['fps b=100 %d->%d' % (n, m)] = fps_row(100, n, m, reps)
    for n in (32768, 131072):
        out['fps b=1 %d->1024' % n] = fps_row(1, n, 1024, reps)

    b = 100
    for n, m, c in ((64, 16, 512), (256, 64, 128), (1024, 256, 128), (1024, 1024, 128)):
        x1 = torch.rand((b, n, 3), generator=g).to(dev)
        x2 = torch.rand((b, m, 3), generator=g).to(dev)
        pts = torch.randn((b, m, c), generator=g).to(dev)
        dist = torch.empty((b, n, 3), device=dev)
        idx = torch.empty((b, n, 3), dtype=torch.int32, device=dev)
        w = torch.full((b, n, 3), 1.0 / 3, device=dev)
        o = torch.empty((b, n, c), device=dev)

        def nn():
            _lib.check(lib.lrg_three_nn(b, n, m, _ptr(x1), _ptr(x2), _ptr(dist), _ptr(idx), _stream_ptr()), 'three_nn')

        def interp():
            _lib.check(lib.lrg_three_interpolate(b, m, c, n, _ptr(pts), _ptr(idx), _ptr(w), _ptr(o), _stream_ptr()), 'three_interpolate')

        def fused():
            _lib.check(lib.lrg_three_nn_interpolate(b, n, m, c, _ptr(x1), _ptr(x2), _ptr(pts), None, None, None, _ptr(o), _stream_ptr()), 'fused')
        nn()
        t_nn, t_in, t_fu = _time_gpu(nn, reps), _time_gpu(interp, reps), _time_gpu(fused, reps)
        evals = b * n * m
        bytes_nn = b * (n + m) * 12 + b * n * 24
        bytes_in = b * m * c * 4 + b * n * 24 + b * n * c * 4
        bytes_fu = b * (n + m) * 12 + b * m * c * 4 + b * n * c * 4
        out['interp b=100 %d<-%d c=%d' % (n, m, c)] = dict(
            b=b, n=n, m=m, c=c,
            three_nn_us=t_nn * 1e6, three_nn_evals=evals, three_nn_frac_of_valu_peak=evals * NN_OPS / t_nn / VALU,
            three_nn_frac_of_hbm_peak=bytes_nn / t_nn / HBM,
            three_interpolate_us=t_in * 1e6, three_interpolate_bytes=bytes_in, three_interpolate_frac_of_hbm_peak=bytes_in / t_in / HBM,
            fused_us=t_fu * 1e6, unfused_us=(t_nn + t_in) * 1e6, fused_bytes=bytes_fu, fused_frac_of_hbm_peak=bytes_fu / t_fu / HBM,
            fused_frac_of_valu_peak=evals * NN_OPS / t_fu / VALU)

    # gather_point at the first set-abstraction level's output (b = 100, 1024 -> 256)
    x = torch.rand((b, 1024, 3), generator=g).to(dev)
    gi = torch.randint(0, 1024, (b, 256), generator=g, dtype=torch.int32).to(dev)
    go = torch.empty((b, 256, 3), device=dev)

    def gather():
        _lib.check(lib.lrg_gather_point(b, 1024, 256, _ptr(x), _ptr(gi), _ptr(go), _stream_ptr()), 'gather')
    t = _time_gpu(gather, reps)
    nbytes = b * 256 * 12 + b * 256 * 4 + b * 1024 * 12
    out['gather_point b=100 1024->256'] = dict(gpu_us=t * 1e6, bytes=nbytes, frac_of_hbm_peak=nbytes / t / HBM,
                                               note='0.4 MB: launch-bound, the HBM fraction is not the limit here')
    out['_meta'] = dict(reps=reps, timing='HIP events round back-to-back launches on preallocated buffers', hbm_Bps=HBM,
                        valu_fp32_ops_per_s=VALU, three_nn_ops_per_eval=NN_OPS, device=torch.cuda.get_device_name(dev))
    return out


if __name__ == '__main__':
    res = sampling_rates()
    if len(sys.argv) > 1:
        json.dump(res, open(sys.argv[1], 'w'), indent=1)
    print(json.dumps(res, indent=1))
