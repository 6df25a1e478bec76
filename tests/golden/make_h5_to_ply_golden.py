"""Golden outputs of the reference's own h5_to_ply.py, produced by running the unmodified script (runpy) on a two-room fixture this
file writes itself: the stub h5py of tf_numpy_standin.py serves the fixture from memory, matplotlib runs on the Agg backend, and the
script works in a temporary directory.

    python tests/golden/make_h5_to_ply_golden.py            # needs the reference checkout (LRG_REFERENCE, default /root/reference)

Writes, under tests/golden/: h5_to_ply_rooms.h5 (the fixture, through h5lite) and h5_to_ply_<run>_<room>.ply with
h5_to_ply_<run>.stdout for the runs rgb (--rgb), seg (--seg) and seg02 (--seg --resolution 0.2).  Data only.

The fixture: two rooms of a few hundred raw points on a jittered lattice, several raw points per voxel (a raw point takes its voxel's first
point's colour), negative coordinates, room 0 with smallest object id 0 (the reference then adds 1 to every id), room 1 with smallest id
2, and in both rooms objects of equal size among the equalised points at resolution 0.1, so that the argsort of the counts has a tie to
break.
"""
import contextlib
import io
import os
import runpy
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('LRG_REFERENCE', '/root/reference')
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

RUNS = {'rgb': ['--rgb'], 'seg': ['--seg'], 'seg02': ['--seg', '--resolution', '0.2']}
SUBDIR = {'rgb': 'rgb', 'seg': 'gt', 'seg02': 'gt'}


def make_room(seed, first_id, origin):
    """Voxel centres on a 0.1 lattice, 1 to 4 raw points in each, jittered by less than 0.04: at resolution 0.1 every cell is a voxel of
    its own and the objects are whole voxels, the second and the third (and the fourth and the fifth) of the same size; at 0.2 cells merge,
    also across objects, and the counts change."""
    rs = np.random.RandomState(seed)
    cells = np.array([(x, y, z) for x in range(6) for y in range(5) for z in range(3)], dtype=np.float64)      # 90 voxels
    cells = cells[rs.permutation(len(cells))]
    sizes = [30, 17, 17, 9, 9, 5, 3]                          # voxels per object: two ties
    obj_of_cell = np.repeat(np.arange(len(sizes)), sizes) + first_id
    cls_of_obj = rs.randint(0, 5, len(sizes))
    rows = []
    for c, o in zip(cells, obj_of_cell):
        for _ in range(rs.randint(1, 5)):
            xyz = origin + c * 0.1 + rs.uniform(-0.04, 0.04, 3)
            rows.append(np.concatenate([xyz, rs.uniform(-0.5, 0.5, 3), [o, cls_of_obj[o - first_id]]]))
    rows = np.array(rows, dtype=np.float32)
    # raw points of different objects share no voxel, but within a voxel the colours differ: file order decides which one the voxel shows
    return rows[rs.permutation(len(rows))]


def main():
    import matplotlib
    matplotlib.use('Agg')
    import tf_numpy_standin as standin
    from learn_region_grow_amd import h5lite
    rooms = [make_room(11, 0, np.array([-1.3, -0.9, 0.0])), make_room(12, 2, np.array([0.5, -2.1, -0.7]))]
    points = np.vstack(rooms).astype(np.float32)
    count = np.array([len(r) for r in rooms], dtype=np.int32)
    h5lite.write_file(os.path.join(HERE, 'h5_to_ply_rooms.h5'), {'points': points, 'count_room': count})
    standin.install()
    sys.path.insert(0, REF)
    for run, flags in RUNS.items():
        with tempfile.TemporaryDirectory() as tmp:
            for sub in ('rgb', 'gt', 'class'):
                os.makedirs(os.path.join(tmp, 'data', sub))
            standin.H5_FILES['rooms.h5'] = {'points': points.copy(), 'count_room': count.copy()}
            argv, cwd, out = sys.argv, os.getcwd(), io.StringIO()
            sys.argv = ['h5_to_ply.py', 'rooms.h5'] + flags
            os.chdir(tmp)
            try:
                with contextlib.redirect_stdout(out):
                    runpy.run_path(os.path.join(REF, 'h5_to_ply.py'), run_name='__main__')
            finally:
                sys.argv = argv
                os.chdir(cwd)
            for r in range(len(rooms)):
                data = open(os.path.join(tmp, 'data', SUBDIR[run], '%d.ply' % r), 'rb').read()
                open(os.path.join(HERE, 'h5_to_ply_%s_%d.ply' % (run, r)), 'wb').write(data)
            open(os.path.join(HERE, 'h5_to_ply_%s.stdout' % run), 'w').write(out.getvalue())
        print(run, [len(r) for r in rooms], out.getvalue().strip().splitlines())


if __name__ == '__main__':
    main()
