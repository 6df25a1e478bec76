#!/usr/bin/env python3
"""Generate tests/golden/baselines_ref_cpu.npz by executing the REFERENCE's benchmarks.py, unmodified, in the build container
(needs the reference checkout; never runs on the GPU box).

    python tests/golden/make_baseline_golden.py [<reference checkout>]

Modes normal, curvature, color, feature and smoothness, each on one room file of three seeded rooms (tests/baselines_ref.py:
golden_rooms): two box rooms of synthetic.generate_room_points (~40 k raw points) and one sparse room of small planar patches,
whose small smoothness regions exercise the duplicate-counting rule of benchmarks.py:384-405.  h5py comes from tf_numpy_standin (as for make_golden.py),
sklearn.externals.joblib is joblib, matplotlib runs on Agg.  The script only prints the metrics of each room, so its
cluster_label of every room is read where it is handed to sklearn.metrics.normalized_mutual_info_score (:463): that name is
wrapped, before the script imports it, by a function that records its arguments and returns the original's result.
Stored: a SHA-256 digest of the rooms (the tests regenerate them from their seeds and check it), cluster_label per (mode, room)
as int16, the thresholds used and the printed metric lines.
"""
import contextlib
import io
import os
import runpy
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import tf_numpy_standin as standin  # noqa: E402
import baselines_ref  # noqa: E402

MODES = ('normal', 'curvature', 'color', 'feature', 'smoothness')
THRESHOLDS = {'normal': (0.99, 0.0, 0.0), 'curvature': (0.01, 0.0, 0.0), 'color': (0.005, 0.0, 0.0),
              'feature': (0.98, 0.1, 0.1), 'smoothness': (0.98, 0.0, 0.0)}        # benchmarks.py:127-142 for --area 5


def run_benchmarks(ref, mode, rooms):
    """benchmarks.py --mode <mode> --area 5 on the room file `rooms`: (cluster_label per room, printed lines)."""
    standin.install()
    import joblib
    import matplotlib
    matplotlib.use('Agg')
    import sklearn.externals  # noqa: F401
    import sklearn.metrics
    sys.modules['sklearn.externals.joblib'] = joblib
    sys.modules.pop('class_util', None)
    standin.H5_FILES.clear()
    standin.H5_FILES['data/s3dis_area5.h5'] = {'points': np.vstack(rooms), 'count_room': np.array([len(r) for r in rooms], dtype=np.int32)}
    labels = []
    orig = sklearn.metrics.normalized_mutual_info_score

    def recording_nmi(obj_id, cluster_label, *args, **kw):
        labels.append(np.array(cluster_label, dtype=np.int32))
        return orig(obj_id, cluster_label, *args, **kw)
    old_argv, old_cwd, old_path = sys.argv, os.getcwd(), list(sys.path)
    buf = io.StringIO()
    try:
        sklearn.metrics.normalized_mutual_info_score = recording_nmi
        os.chdir(ref)
        sys.path.insert(0, ref)
        sys.argv = ['benchmarks.py', '--mode', mode, '--area', '5']
        with contextlib.redirect_stdout(buf):
            g = runpy.run_path(os.path.join(ref, 'benchmarks.py'), run_name='__main__')
    finally:
        sklearn.metrics.normalized_mutual_info_score = orig
        sys.argv = old_argv
        os.chdir(old_cwd)
        sys.path[:] = old_path
    used = (g['threshold'], g.get('threshold2', 0.0), g.get('threshold3', 0.0))
    assert tuple(used) == THRESHOLDS[mode], (mode, used)
    assert len(labels) == len(rooms) and all(0 <= l.max() < 2 ** 15 for l in labels)
    return labels, buf.getvalue().rstrip('\n').split('\n')


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'
    rooms = baselines_ref.golden_rooms()
    out = {'rooms_digest': np.array(baselines_ref.rooms_digest(rooms))}
    small_kept = 0
    for mode in MODES:
        labels, lines = run_benchmarks(ref, mode, rooms)
        for r, lab in enumerate(labels):
            out['%s__label%d' % (mode, r)] = lab.astype(np.int16)      # ids stay far below 2^15
            if mode == 'smoothness':
                ids, cnt = np.unique(lab[lab > 0], return_counts=True)
                small_kept += int((cnt <= 10).sum())
        out[mode + '__thresholds'] = np.array(THRESHOLDS[mode])
        out[mode + '__room_lines'] = np.array([l for l in lines if l.startswith('Area ')])
        out[mode + '__aggregate_line'] = np.array(lines[-1])
        print(mode, [int(l.max()) for l in labels], lines[-1])
    # the duplicate-counting rule must decide at least one region: a kept region of at most 10 distinct points
    assert small_kept > 0, 'no smoothness region of <= 10 distinct points was kept: the golden would not cover the replay'
    path = os.path.join(HERE, 'baselines_ref_cpu.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, '(%d smoothness regions of <= 10 points kept)' % small_kept)


if __name__ == '__main__':
    main()
