"""Helpers shared by the GPU tests of the PointNet and PointNet2 trainers (test_gpu_pointnet_train.py, test_gpu_pointnet2_train.py,
test_gpu_trainer_bits.py).  A plain module: no fixtures, no test."""
import numpy as np

f32 = np.float32
P = 1024


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def adam_f32(p, g, m, v, lr_t, b1, b2, eps):
    """lrg_adam_kernel's expression, operation by operation, in NumPy float32 -> (p, m, v)."""
    lr_t, b1, b2, eps, one = f32(lr_t), f32(b1), f32(b2), f32(eps), f32(1)
    m2 = m + (g - m) * (one - b1)
    v2 = v + (g * g - v) * (one - b2)
    return p - lr_t * m2 / (np.sqrt(v2) + eps), m2, v2


def three_cells(seed):
    """1024 distinct points; about 300 distinct points drawn with replacement (ball-query padding and pool ties are routine); one
    point 1024 times."""
    rs = np.random.RandomState(seed)
    def cloud(n):
        p = rs.uniform(-0.5, 0.5, (n, 6)).astype(f32)
        p[:, 2] = rs.uniform(0, 2.5, n)
        p[:, 3:] = rs.uniform(0, 1, (n, 3))
        return p
    few = cloud(300)
    return np.stack([cloud(P), few[np.concatenate([np.arange(300), rs.randint(0, 300, P - 300)])], np.repeat(cloud(1), P, axis=0)])
