"""The rooms of tests/test_gpu_preprocess_batch.py, one lrg_preprocess call at the C-ABI, and the digests of what it writes: shared by
the tests and by tools/prep_golden_digests.py, which records tests/golden/preprocess_single_room.json."""
import ctypes
import hashlib

import numpy as np

from learn_region_grow_amd import synthetic

DIGEST_F = (6, 9, 12, 13)
DIGEST_MODES = (0, 1, 2)


def raw_room(seed, n=2500, wlh=(1.6, 1.3, 1.0)):
    r = synthetic.generate_room_points(n, seed, wlh=wlh).astype(np.float32)
    return r[:, :6], r[:, 6].astype(int), r[:, 7].astype(int)


def degenerate_room():
    """tests/test_gpu_preprocess.py::test_degenerate_inputs: one crowded voxel and isolated points (NaN curvature)."""
    rs = np.random.RandomState(0)
    raw = np.zeros((400, 6), np.float32)
    raw[:300, :3] = 0.5 + rs.rand(300, 3) * 0.04
    raw[300:, :3] = rs.rand(100, 3) * 3
    raw[:, 3:6] = rs.rand(400, 3)
    obj = np.arange(400) % 7
    return raw, obj, obj


def six_rooms():
    """Twice the same room (same voxels: the two must not see each other), two more, a single point, the degenerate room."""
    one = raw_room(1)
    return [one, (one[0].copy(), one[1].copy(), one[2].copy()), raw_room(2), raw_room(3), (one[0][:1], one[1][:1], one[2][:1]), degenerate_room()]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def capi_single(lib, dev, room, F, mode):
    """lrg_preprocess on one room: everything it writes, as it writes it."""
    import torch
    raw_np = np.ascontiguousarray(room[0][:, :6], np.float32)
    M = len(raw_np)
    raw = torch.from_numpy(raw_np).to(dev)
    obj = torch.from_numpy(np.ascontiguousarray(room[1], np.int32)).to(dev)
    cls = torch.from_numpy(np.ascontiguousarray(room[2], np.int32)).to(dev)
    ws = torch.empty(lib.lrg_preprocess_workspace_bytes(M), dtype=torch.uint8, device=dev)
    eq, uneq, n_dev = (torch.empty(M, dtype=torch.int32, device=dev) for _ in range(3))
    pts = torch.empty((M, F), dtype=torch.float32, device=dev)
    obj_o, cls_o, nflag = (torch.empty(M, dtype=torch.int32, device=dev) for _ in range(3))
    curv = torch.empty(M, dtype=torch.float64, device=dev)
    cov = torch.empty((M, 9), dtype=torch.float64, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.lrg_preprocess(_ptr(raw), 6, _ptr(obj), _ptr(cls), M, ctypes.c_float(0.1), F, mode, _ptr(ws), ws.numel(), _ptr(pts), _ptr(obj_o),
                              _ptr(cls_o), _ptr(curv), _ptr(eq), _ptr(uneq), _ptr(cov), _ptr(n_dev), st) == 0
    N = int(n_dev[0].item())
    out = dict(eq=eq[:N], uneq=uneq, cov=cov[:N])
    if mode:
        out.update(points=pts[:N], obj=obj_o[:N], cls=cls_o[:N], curv=curv[:N])
    if mode == 2:
        assert lib.lrg_preprocess_unsafe_normals(_ptr(ws), M, N, _ptr(nflag), st) == 0
        out['unsafe'] = nflag[:N]
    return {k: v.cpu().numpy() for k, v in out.items()}


def hipcc_version():
    """The compiler that builds the library: the digests depend on it."""
    import subprocess
    from learn_region_grow_amd import _lib
    return subprocess.check_output([_lib.hipcc_and_flags()[0], '--version'], text=True).strip()


def digest_key(F, mode, room):
    return 'F%d/eig_mode%d/room%d' % (F, mode, room)


def digests(arrays, mode):
    """sha256 of the raw bytes of every array one call wrote for a room (eig_mode 1 writes no covariances)."""
    return {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in sorted(arrays.items()) if not (k == 'cov' and mode == 1)}
