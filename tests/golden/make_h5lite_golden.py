#!/usr/bin/env python3
"""Generate h5lite_written.h5: the file learn_region_grow_amd.h5lite.write_file writes for tests/test_formats.py, checked here by
h5py (run it with an interpreter that has h5py and NumPy):
    python3 tests/golden/make_h5lite_golden.py
tests/test_formats.py then asserts that the writer still produces these bytes.
"""
import os
import sys

import h5py
import numpy as np

here = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(here)))
from learn_region_grow_amd import h5lite  # noqa: E402

z = np.load(os.path.join(here, 'rooms_expected.npz'))
path = os.path.join(here, 'h5lite_written.h5')
h5lite.write_file(path, {'points': z['points'], 'count_room': z['count_room'], 'f64': np.arange(7.0),
                         'i8': np.arange(5, dtype=np.int8), 'empty': np.zeros((0, 8), np.float32)})
with h5py.File(path, 'r') as f:
    assert sorted(f.keys()) == ['count_room', 'empty', 'f64', 'i8', 'points'], list(f.keys())
    assert f['points'].dtype == np.float32 and np.array_equal(f['points'][:], z['points'])
    assert f['count_room'].dtype == np.int32 and np.array_equal(f['count_room'][:], z['count_room'])
    assert np.array_equal(f['f64'][:], np.arange(7.0)) and np.array_equal(f['i8'][:], np.arange(5))
    assert f['empty'].shape == (0, 8)
print('wrote and checked', path)
