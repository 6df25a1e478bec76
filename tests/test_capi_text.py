"""CPU: the text encoder's entries exist in the built library and its constants agree between the header and the binding."""
import ctypes
import os
import re

from conftest import REPO
from learn_region_grow_amd import _lib


def test_text_symbols_and_constants(hip_lib):
    for name in ('lrg_text_encode', 'lrg_text_workspace_bytes'):
        assert name in _lib.EXPORTS and hasattr(hip_lib, name)
    header = open(os.path.join(REPO, 'include', 'lrg_hip.h')).read()
    const = {k: int(v) for k, v in re.findall(r'#define\s+(LRG_TEXT_\w+)\s+(\d+)', header)}
    assert const == dict(LRG_TEXT_MAX_LINE=_lib.LRG_TEXT_MAX_LINE, LRG_TEXT_PLY=_lib.LRG_TEXT_PLY, LRG_TEXT_PCD=_lib.LRG_TEXT_PCD)
    assert 'lrg_text.hip' in _lib.SOURCES
    from learn_region_grow_amd import io as lio
    assert lio.TEXT_FORMATS == dict(ply=_lib.LRG_TEXT_PLY, pcd=_lib.LRG_TEXT_PCD)
    assert lio.text_rows_per_call() * _lib.LRG_TEXT_MAX_LINE < 2 ** 31 <= (lio.text_rows_per_call() + 1) * _lib.LRG_TEXT_MAX_LINE


def test_text_entry_refuses_before_any_launch(hip_lib):
    """The argument checks come before anything touches the device, so they run without one."""
    ws = hip_lib.lrg_text_workspace_bytes(1000)
    assert ws >= 1001 * 4 and hip_lib.lrg_text_workspace_bytes(0) > 0
    p = ctypes.c_void_p(4096)                                    # never dereferenced: every call below is refused
    enc = hip_lib.lrg_text_encode
    big = (2 ** 31) // _lib.LRG_TEXT_MAX_LINE + 1
    assert enc(p, 3, p, 10, 0, None, 1 << 20, p, p, 1 << 20, p, None) == _lib.LRG_EINVAL - 130
    assert enc(p, 3, p, 10, 0, p, 1 << 20, p, ctypes.c_void_p(4100), 1 << 20, p, None) == _lib.LRG_EINVAL - 130      # text not 16-byte aligned
    assert enc(p, 3, p, -1, 0, p, 1 << 20, p, p, 1 << 20, p, None) == _lib.LRG_EINVAL - 131
    assert enc(p, 3, p, big, 0, p, 1 << 40, p, p, 1 << 40, p, None) == _lib.LRG_EINVAL - 131
    assert enc(p, 2, p, 10, 0, p, 1 << 20, p, p, 1 << 20, p, None) == _lib.LRG_EINVAL - 132
    assert enc(p, 3, p, 10, 2, p, 1 << 20, p, p, 1 << 20, p, None) == _lib.LRG_EINVAL - 133
    assert enc(p, 3, p, 10, 0, p, 16, p, p, 1 << 20, p, None) == _lib.LRG_EINVAL - 134
    assert enc(p, 3, p, 10, 0, p, 1 << 20, p, p, 10 * _lib.LRG_TEXT_MAX_LINE - 1, p, None) == _lib.LRG_EINVAL - 134
