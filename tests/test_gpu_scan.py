"""GPU: the exclusive scan that preprocessing, the baselines and MCPNet's candidate lists share (csrc/lrg_scan.hip: lrg_exscan_i32;
declared in csrc/lrg_common.h, not part of include/lrg_hip.h), driven directly.  A block is 2048 elements and the kernel that scans
the block sums handles 256 of them per trip of its loop: 2048 is one block, 524288 the last length of one trip, 524289 the first
that carries into a second.  No caller scans in place, so no case does."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
BLOCK = 2048
LENGTHS = [1, 63, 64, 65, 2047, 2048, 2049, 524288, 524289, 524288 + 3 * 2048 + 5]


@pytest.fixture(scope='module')
def exscan(cuda_device):
    import torch
    from learn_region_grow_amd import _lib
    fn = ctypes.CDLL(_lib.LIB_PATH).lrg_exscan_i32
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]

    def run(x, n, out_fill=-7):
        """(return code, out, bsum) of a scan of the first n of x; out and bsum start as out_fill"""
        nb = (n + BLOCK - 1) // BLOCK
        dx = torch.from_numpy(x).to(cuda_device)
        out = torch.full((max(n, 1),), out_fill, dtype=torch.int32, device=cuda_device)
        bsum = torch.full((nb + 1,), out_fill, dtype=torch.int32, device=cuda_device)
        rc = fn(dx.data_ptr(), n, bsum.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc, out.cpu().numpy(), bsum.cpu().numpy()
    return run


@pytest.mark.parametrize('n', LENGTHS)
def test_exclusive_scan_and_total(exscan, n):
    x = np.random.RandomState(n).randint(0, 4, size=n).astype(np.int32)
    rc, out, bsum = exscan(x, n)
    assert rc == 0
    assert np.array_equal(out, np.cumsum(x, dtype=np.int64) - x)
    assert bsum[(n + BLOCK - 1) // BLOCK] == x.sum()


def test_empty_scan_launches_nothing(exscan):
    rc, out, bsum = exscan(np.ones(1, np.int32), 0)
    assert rc == 0
    assert np.all(out == -7) and np.all(bsum == -7)
