"""NumPy restatement of the edge certificate (lrg_baseline_certify) and the hand-made rooms that pin it.

``certify`` walks the pairs k < i of the 26-neighbour voxel graph like the kernel and evaluates each conjunct with the operations the
kernel uses, in its order:
  normal      d = fma(a2, b2, fma(a1, b1, a0 * b0));  E_n = ((2 (s_i + s_k)) + ((3 s_i) s_k)) + 8 eps;  certain iff |d - t| > 2 E_n
  curvature   v = |c_k - c_i|;                         E_c = (sc_i + sc_k) + 2 eps;                    certain iff |v - t| > 2 E_c
  colour      always certain (float32 arithmetic on the raw data)
An edge is uncertain when a conjunct is uncertain and none is certainly false; both its ends are flagged.

``handmade`` builds two rooms whose named edges sit exactly on the boundaries of those inequalities; the values are built from the
thresholds with exact float64 arithmetic, and ``handmade`` itself asserts that every sum and difference it relies on is exact.
"""
import numpy as np

import baselines_ref as R

EPS = float(np.finfo(np.float64).eps)
T_NORMAL, T_CURV, T_COLOR = 0.125, 0.75, 0.1
SLACK = 2.0 ** -4            # room B: large enough for 2 E to have the ulp of the values it is added to
CERT_MODES = ('normal', 'curvature', 'feature', 'smoothness')


def thresholds(mode):
    """The thresholds the hand-made rooms are written for."""
    return {'normal': (T_NORMAL, 0.0, 0.0), 'smoothness': (T_NORMAL, 0.0, 0.0), 'curvature': (T_CURV, 0.0, 0.0),
            'feature': (T_NORMAL, T_CURV, T_COLOR), 'color': (T_COLOR, 0.0, 0.0)}[mode]


def e_normal(si, sk):
    return ((2.0 * (si + sk)) + ((3.0 * si) * sk)) + 8.0 * EPS


def e_curv(si, sk):
    return (si + sk) + 2.0 * EPS


def _normal_conjunct(room, i, k, t):
    """0 certainly false, 1 certainly true, 2 uncertain."""
    with np.errstate(invalid='ignore'):
        d = R.ddot3(room['normals'][k], room['normals'][i])
        e = e_normal(float(room['normal_slack'][i]), float(room['normal_slack'][k]))
        if not abs(d - t) > 2.0 * e:
            return 2
    return 1 if d > t else 0


def _curv_conjunct(room, i, k, t):
    with np.errstate(invalid='ignore'):
        v = abs(float(room['curvatures'][k]) - float(room['curvatures'][i]))
        e = e_curv(float(room['curv_slack'][i]), float(room['curv_slack'][k]))
        if not abs(v - t) > 2.0 * e:
            return 2
    return 1 if v < t else 0


def edge_uncertain(room, mode, t, i, k):
    if mode in ('normal', 'smoothness'):
        return _normal_conjunct(room, i, k, t[0]) == 2
    if mode == 'curvature':
        return _curv_conjunct(room, i, k, t[0]) == 2
    if mode == 'feature':
        cn, cc = _normal_conjunct(room, i, k, t[0]), _curv_conjunct(room, i, k, t[1])
        colour = bool(R.color_edge(room['points'], np.array([i]), np.array([k]), t[2])[0])
        if cn == 0 or cc == 0 or not colour:
            return False
        return cn == 2 or cc == 2
    raise ValueError(mode)


def certify(room, mode, t, resolution=0.1):
    """flags [n] bool of one room: both ends of every uncertain edge."""
    n = len(room['points'])
    flags = np.zeros(n, dtype=bool)
    if mode == 'color':
        return flags
    nb = R.neighbours(room['points'], resolution)
    for i in range(n):
        for k in nb[i]:
            if 0 <= k < i and edge_uncertain(room, mode, t, i, int(k)):
                flags[i] = flags[k] = True
    return flags


def _room(voxels):
    n = len(voxels)
    xyz = (np.asarray(voxels, dtype=np.float64) * 0.1).astype(np.float32)
    rgb = np.full((n, 3), 0.5, dtype=np.float32)
    normals = np.tile([0.0, 0.0, 1.0], (n, 1))                       # d(i, k) = z_i z_k, exact where one of them is 1
    small = 2.0 ** -30
    return dict(points=np.hstack([xyz, rgb]).astype(np.float32), normals=normals, curvatures=np.zeros(n), rank=np.arange(n, dtype=np.int32),
                normal_slack=np.full(n, small), curv_slack=np.full(n, small))


def handmade():
    """(rooms, expected): rooms A and B; expected[mode] = [flags of A, flags of B] as worked out by hand below.

    Room A: the voxel block {0, 1, 2}^3 (point 9 x + 3 y + z) and a tail at (3, 3, 3) (point 27) whose only neighbour is corner 26.
    Every other pair is certainly an edge (d = 1 against 0.125, |dc| = 0 against 0.75, one colour), except where a point is named:
      point 0   infinite slacks: its edges to the 7 other points of {0, 1}^3 are uncertain
      point 8   (0, 2, 2) NaN normal and curvature, finite slacks: likewise for x in {0, 1}, y, z in {1, 2}
      point 18  (2, 0, 0) normal z = T_NORMAL, so d == t on all 7 edges (uncertain), and a colour of its own: in mode 'feature' the
                colour conjunct of those edges is false and nothing is flagged for them; its curvature is certain
      26 - 27   slack 0 at both ends, d == t and |dc| == t: uncertain (8 eps, 2 eps remain)
    Room B: voxels (0..4, 0, 0), every slack 2^-4; points 1, 2, 4 plain.
      0 - 1     |d - t| = 2 E_n and ||dc| - t| = 2 E_c exactly: uncertain
      2 - 3 and 3 - 4   the next double above 2 E: certain (true), and 1 - 2 is far from both thresholds: 2, 3, 4 stay unflagged
    """
    A = _room([(x, y, z) for x in range(3) for y in range(3) for z in range(3)] + [(3, 3, 3)])
    A['normal_slack'][0] = A['curv_slack'][0] = np.inf
    A['normals'][8] = np.nan
    A['curvatures'][8] = np.nan
    A['normals'][18, 2] = T_NORMAL
    A['points'][18, 3:6] = (0.0, 1.0, 0.0)
    A['normal_slack'][[26, 27]] = 0.0
    A['curv_slack'][[26, 27]] = 0.0
    A['normals'][27, 2] = T_NORMAL
    A['curvatures'][27] = T_CURV
    B = _room([(x, 0, 0) for x in range(5)])
    B['normal_slack'][:] = SLACK
    B['curv_slack'][:] = SLACK
    two_en, two_ec = 2.0 * e_normal(SLACK, SLACK), 2.0 * e_curv(SLACK, SLACK)
    up_n, up_c = float(np.nextafter(two_en, np.inf)), float(np.nextafter(two_ec, np.inf))
    B['normals'][0, 2] = T_NORMAL + two_en
    B['normals'][3, 2] = T_NORMAL + up_n
    B['curvatures'][0] = T_CURV - two_ec
    B['curvatures'][3] = T_CURV - up_c
    # every value above is what it is meant to be, to the bit
    assert abs(R.ddot3(B['normals'][0], B['normals'][1]) - T_NORMAL) == two_en
    assert abs(R.ddot3(B['normals'][3], B['normals'][2]) - T_NORMAL) == up_n > two_en
    assert abs(abs(B['curvatures'][1] - B['curvatures'][0]) - T_CURV) == two_ec
    assert abs(abs(B['curvatures'][3] - B['curvatures'][2]) - T_CURV) == up_c > two_ec
    assert R.ddot3(A['normals'][27], A['normals'][26]) == T_NORMAL and abs(A['curvatures'][27] - A['curvatures'][26]) == T_CURV

    def block(xs, ys, zs):
        return {9 * x + 3 * y + z for x in xs for y in ys for z in zs}
    s_inf, s_nan, s_18, s_tail = block((0, 1), (0, 1), (0, 1)), block((0, 1), (1, 2), (1, 2)), block((1, 2), (0, 1), (0, 1)), {26, 27}

    def flags(n, idx):
        f = np.zeros(n, dtype=bool)
        f[sorted(idx)] = True
        return f
    b = flags(5, {0, 1})
    expected = {'normal': [flags(28, s_inf | s_nan | s_18 | s_tail), b], 'curvature': [flags(28, s_inf | s_nan | s_tail), b],
                'feature': [flags(28, s_inf | s_nan | s_tail), b], 'color': [flags(28, ()), flags(5, ())]}
    expected['smoothness'] = expected['normal']
    return [A, B], expected
