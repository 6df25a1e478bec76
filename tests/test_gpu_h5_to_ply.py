"""GPU: h5_to_ply.py and examine_h5.py as child processes against what the reference's own h5_to_ply.py wrote for the same room file
(tests/golden/make_h5_to_ply_golden.py), byte for byte; --cls and --target, whose tables the reference keeps in its program text, against
a NumPy restatement of h5_to_ply.py:72-111 here."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO
from learn_region_grow_amd import io as lio

pytestmark = pytest.mark.gpu
ROOMS = os.path.join(GOLDEN, 'h5_to_ply_rooms.h5')
TABLE = ['0 clutter 10 20 30', '1 chair 200 0 0', '2 ceiling 0 200 0', '3 table 0 0 200', '4 wall 255 255 1']


def _run(script, args, cwd):
    r = subprocess.run([sys.executable, os.path.join(REPO, script)] + args, capture_output=True, text=True, cwd=str(cwd), timeout=300)
    return r


@pytest.mark.parametrize('run,flags,sub', [('rgb', ['--rgb'], 'rgb'), ('rgb', [], 'rgb'), ('seg', ['--seg'], 'gt'),
                                           ('seg02', ['--seg', '--resolution', '0.2'], 'gt')])
def test_files_and_lines_equal_the_reference(cuda_device, tmp_path, run, flags, sub):
    r = _run('h5_to_ply.py', [ROOMS] + flags, tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == open(os.path.join(GOLDEN, 'h5_to_ply_%s.stdout' % run)).read()          # 'Saved to data/gt/0.ply: (223 points)'
    for room in range(2):
        got = open(tmp_path / 'data' / sub / ('%d.ply' % room), 'rb').read()
        assert got == open(os.path.join(GOLDEN, 'h5_to_ply_%s_%d.ply' % (run, room)), 'rb').read(), room
    assert sorted(os.listdir(tmp_path / 'data')) == [sub]


def test_out_directory(cuda_device, tmp_path):
    r = _run('h5_to_ply.py', [ROOMS, '--seg', '--out', 'clouds/deep'], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == open(os.path.join(GOLDEN, 'h5_to_ply_seg.stdout')).read().replace('data/gt', 'clouds/deep/gt')
    assert open(tmp_path / 'clouds' / 'deep' / 'gt' / '1.ply', 'rb').read() == open(os.path.join(GOLDEN, 'h5_to_ply_seg_1.ply'), 'rb').read()


def _equalize(points, resolution=0.1):
    """h5_to_ply.py:72-81"""
    equalized_idx, unequalized_idx, seen = [], [], {}
    for i in range(len(points)):
        k = tuple(np.round(points[i, :3] / resolution).astype(int))
        if k not in seen:
            seen[k] = len(equalized_idx)
            equalized_idx.append(i)
        unequalized_idx.append(seen[k])
    return np.array(equalized_idx), np.array(unequalized_idx)


def test_class_colours_from_a_table(cuda_device, tmp_path, capsys):
    (tmp_path / 'classes.txt').write_text('# id name r g b\n' + '\n'.join(TABLE) + '\n')
    r = _run('h5_to_ply.py', [ROOMS, '--cls', '--class-table', 'classes.txt'], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    colour = np.array([[int(v) for v in ln.split()[2:]] for ln in TABLE])
    rooms, _, cls = lio.loadFromH5(ROOMS)
    want_out = ''
    for room in range(2):
        eq, uneq = _equalize(rooms[room])
        pts = rooms[room].copy()
        pts[:, 3:6] = colour[cls[room][eq][uneq]]                  # :111
        lio.savePLY(str(tmp_path / ('want%d.ply' % room)), pts)
        capsys.readouterr()
        want_out += 'Saved to data/class/%d.ply: (%d points)\n' % (room, len(pts))
        assert open(tmp_path / 'data' / 'class' / ('%d.ply' % room), 'rb').read() == open(tmp_path / ('want%d.ply' % room), 'rb').read(), room
    assert r.stdout == want_out


def test_class_colours_need_a_table(cuda_device, tmp_path):
    r = _run('h5_to_ply.py', [ROOMS, '--cls'], tmp_path)
    assert r.returncode != 0 and '--class-table' in r.stderr
    assert not os.path.exists(tmp_path / 'data')
    (tmp_path / 'short.txt').write_text('\n'.join(TABLE[:3]) + '\n')          # class ids 3 and 4 of the file are not named
    r = _run('h5_to_ply.py', [ROOMS, '--cls', '--class-table', 'short.txt'], tmp_path)
    assert r.returncode != 0 and 'class table' in r.stderr


@pytest.mark.parametrize('with_table', [True, False])
def test_target_legend(cuda_device, tmp_path, with_table):
    (tmp_path / 'classes.txt').write_text('\n'.join(TABLE) + '\n')
    r = _run('h5_to_ply.py', [ROOMS, '--target', '0'] + (['--class-table', 'classes.txt'] if with_table else []), tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    names = {int(ln.split()[0]): ln.split()[1] for ln in TABLE} if with_table else {}
    rooms, obj, cls = lio.loadFromH5(ROOMS)
    eq, _ = _equalize(rooms[0])
    obj_id, cls_id = obj[0][eq], cls[0][eq]
    assert obj_id.min() == 0
    obj_id = obj_id + 1                                                         # :90-91
    obj_color = np.random.RandomState(0).randint(0, 255, (obj_id.max() + 1, 3))
    unique_id, count = np.unique(obj_id, return_counts=True)
    assert len(set(count.tolist())) < len(count)                                # the fixture's tie
    want = []
    for k in range(len(unique_id)):
        i = unique_id[np.argsort(count)][::-1][k]
        c = int(cls_id[np.nonzero(obj_id == i)[0][0]])
        name = names.get(c, 'class %d' % c)
        if name not in ('ceiling', 'none', 'unlabeled'):
            want.append('%s #%d: %d %d %d' % (name, k, obj_color[k + 1][0], obj_color[k + 1][1], obj_color[k + 1][2]))
    assert r.stdout.splitlines() == want and len(want) >= 3
    if with_table:
        assert len(want) < len(unique_id) or 2 not in cls_id                    # 'ceiling' is left out of the legend
    assert not os.path.exists(tmp_path / 'data')


def test_examine_h5(tmp_path):
    r = _run('examine_h5.py', [os.path.join(GOLDEN, 'rooms_gzip.h5')], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(os.path.join(GOLDEN, 'rooms_expected.npz'))
    lines = r.stdout.splitlines()
    assert lines[0] == '<HDF5 dataset "count_room": shape (%d,), type "<i4">' % len(z['count_room'])
    assert lines[2] == '<HDF5 dataset "points": shape (162, 8), type "<f4">'
    assert lines[1] == 'min %.2f mean %.2f max %.2f' % (z['count_room'].min(), z['count_room'].mean(), z['count_room'].max())
    assert lines[3] == 'min %.2f mean %.2f max %.2f' % (z['points'].min(), z['points'].mean(), z['points'].max())
    assert len(lines) == 4
