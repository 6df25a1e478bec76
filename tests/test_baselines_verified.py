"""CPU: the NumPy restatement of the edge certificate (tests/baselines_verified_ref.py) gives the flags worked out by hand on the
hand-made rooms, and the command line parses --features."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import REPO
import baselines_verified_ref as V


@pytest.mark.parametrize('mode', V.CERT_MODES + ('color',))
def test_restatement_known_answers(mode):
    rooms, expected = V.handmade()
    for room, want in zip(rooms, expected[mode]):
        got = V.certify(room, mode, V.thresholds(mode))
        assert np.array_equal(got, want), (mode, np.nonzero(got != want)[0])


def test_boundary_is_one_ulp_wide():
    """The edge at 2 E exactly is uncertain and the one a double further is not: moving either by one ulp swaps the outcome."""
    rooms, _ = V.handmade()
    B = rooms[1]
    t = V.thresholds('normal')
    assert V.edge_uncertain(B, 'normal', t, 1, 0) and not V.edge_uncertain(B, 'normal', t, 3, 2)
    B['normals'][0, 2] = np.nextafter(B['normals'][0, 2], np.inf)
    B['normals'][3, 2] = np.nextafter(B['normals'][3, 2], -np.inf)
    assert not V.edge_uncertain(B, 'normal', t, 1, 0) and V.edge_uncertain(B, 'normal', t, 3, 2)
    t = V.thresholds('curvature')
    assert V.edge_uncertain(B, 'curvature', t, 1, 0) and not V.edge_uncertain(B, 'curvature', t, 3, 2)
    B['curvatures'][0] = np.nextafter(B['curvatures'][0], -np.inf)
    B['curvatures'][3] = np.nextafter(B['curvatures'][3], np.inf)
    assert not V.edge_uncertain(B, 'curvature', t, 1, 0) and V.edge_uncertain(B, 'curvature', t, 3, 2)


def test_feature_edge_with_false_colour_is_certain():
    rooms, _ = V.handmade()
    A = rooms[0]
    assert V.edge_uncertain(A, 'normal', V.thresholds('normal'), 18, 9)
    assert not V.edge_uncertain(A, 'feature', V.thresholds('feature'), 18, 9)
    A['points'][18, 3:6] = A['points'][9, 3:6]                       # the same colour: the normal conjunct decides again
    assert V.edge_uncertain(A, 'feature', V.thresholds('feature'), 18, 9)


def _cli():
    spec = importlib.util.spec_from_file_location('baselines_cli', os.path.join(REPO, 'baselines.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_features_option():
    cli = _cli()
    assert cli.parse([]).features == 'lapack'
    assert cli.parse(['--features', 'lapack']).features == 'lapack'
    assert cli.parse(['--mode', 'smoothness', '--features', 'verified']).features == 'verified'
    with pytest.raises(SystemExit):
        cli.parse(['--features', 'jacobi'])
