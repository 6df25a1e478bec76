"""CPU: the stages in which PointNet2Trainer adds the rows of a bias gradient (pointnet2_train._colsum_plan), for the row counts of
the network's levels and a prime."""
import numpy as np
import pytest

import conftest  # noqa: F401  (puts the repository on sys.path)

MAX_SEGMENTS = 65535             # lrg_segment_colsum rejects more (test_gpu_train_kernels.py::test_segment_colsum_rejects_too_many_segments)


def level_rows(B):
    from learn_region_grow_amd.pointnet2 import NSAMPLE, NUM_POINT, SA_LEVELS
    npts = [NUM_POINT] + [m for m, _ in SA_LEVELS]
    return sorted(set([B * n * NSAMPLE for n in npts[1:]] + [B * n for n in npts]))


@pytest.mark.parametrize('R', sorted(set(level_rows(1) + level_rows(3) + level_rows(100) + [1, 65521, 1000003])))
def test_stages_multiply_to_the_rows_and_chain(R):
    from learn_region_grow_amd.pointnet2_train import _colsum_plan
    plan = _colsum_plan(R)
    assert int(np.prod([rows for _, rows in plan], dtype=np.int64)) == R
    left = R
    for segs, rows in plan:
        assert rows >= 1 and left % rows == 0 and segs == left // rows, (plan, left)       # the segments are the rows the next stage reads
        assert segs <= MAX_SEGMENTS, plan
        left = segs
    assert left == 1


def test_the_two_trainers_plans_at_three_cells():
    """B * 1024 rows at B = 3 and B = 1: not PointNetTrainer's [(B, 1024), (1, B)].  The two plans differ in bits and stay apart."""
    from learn_region_grow_amd.pointnet2_train import _colsum_plan
    assert _colsum_plan(3 * 1024) == [(12, 256), (3, 4), (1, 3)]
    assert _colsum_plan(1024) == [(4, 256), (1, 4)]
