"""GPU: lrg_text_encode and the io functions built on it write, byte for byte, what io.savePLY / io.savePCD write (tests/test_formats.py
pins those two to the reference's own output)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from learn_region_grow_amd import io as lio

pytestmark = pytest.mark.gpu

HEADER_LINES = {'ply': 10, 'pcd': 11}


def _host_body(tmp_path, xyz, rgb, fmt, name='host'):
    """The bytes of the host file behind its header."""
    path = str(tmp_path / ('%s.%s' % (name, fmt)))
    pts = np.hstack([np.asarray(xyz, dtype=np.float32)[:, :3].astype(np.float64), np.asarray(rgb).astype(np.float64)])
    (lio.savePLY if fmt == 'ply' else lio.savePCD)(path, pts)
    data = open(path, 'rb').read()
    return b''.join(data.splitlines(keepends=True)[HEADER_LINES[fmt]:]), data


def _crafted():
    """About 4 k rows of coordinates where '%f' is hard: signed zeros, exact ties of both parities and their neighbours, carries that
    grow the digit count, subnormals, the largest encoded magnitude."""
    f32 = np.float32
    odd = (np.arange(1, 1200, 2) / 128.0).astype(f32)                                  # exact ties; the kept digit is even for some, odd for others
    kept = (np.floor(odd.astype(np.float64) * 1e6).astype(np.int64)) & 1
    assert kept.min() == 0 and kept.max() == 1
    vals = [np.array([0.0, -0.0, 4.9999997e-7, 5e-7, 0.9999995, 9.9999995, 999999.97, 1e-45, 1e-40, 1.17549435e-38, 2.0 ** 39,
                      2.0 ** 40 - 2.0 ** 16, 123456.789, 1e-9], dtype=f32),
            odd, np.nextafter(odd, f32(np.inf)), np.nextafter(odd, f32(-np.inf)), odd * f32(64.0), np.nextafter(odd * f32(64.0), f32(np.inf))]
    v = np.concatenate(vals)
    v = np.concatenate([v, -v])
    rs = np.random.RandomState(3)
    n = 4099
    v = np.concatenate([v, (rs.randn(max(0, 3 * n - len(v))) * 5).astype(f32)])[:3 * n]
    xyz = v[rs.permutation(3 * n)].reshape(n, 3)
    xyz[0] = [0.0, -0.0, 2.0 ** 40 - 2.0 ** 16]
    return xyz


def _colours(n, fmt, seed=5):
    rs = np.random.RandomState(seed)
    if fmt == 'pcd':
        c = rs.randint(0, 256, (n, 3)).astype(np.int32)
        c[:2] = [[0, 0, 0], [255, 255, 255]]
        return c
    c = rs.choice(np.array([-2 ** 31, -1, 0, 255, 2 ** 31 - 1, 7, 100, 99999], dtype=np.int64), (n, 3)).astype(np.int32)
    c[:1] = [[-2 ** 31, -2 ** 31, -2 ** 31]]
    return c


@pytest.fixture(scope='module')
def crafted(cuda_device, tmp_path_factory):
    """The crafted rows and their host file bodies, computed once."""
    tmp = tmp_path_factory.mktemp('text_host')
    xyz = _crafted()
    out = dict(xyz=xyz)
    for fmt in ('ply', 'pcd'):
        rgb = _colours(len(xyz), fmt)
        body, _ = _host_body(tmp, xyz, rgb, fmt)
        lines = body.splitlines(keepends=True)
        assert len(lines) == len(xyz)
        out[fmt] = (rgb, lines)
    return out


@pytest.mark.parametrize('fmt', ['ply', 'pcd'])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 257, 4099])
def test_crafted_rows_equal_the_host_file(cuda_device, crafted, fmt, n):
    import torch
    rgb, lines = crafted[fmt]
    # rows from the END of the crafted set for the short counts too, so that every count sees different rows and different line lengths
    xyz, rgb, lines = crafted['xyz'][-n:], rgb[-n:], lines[-n:]
    d_xyz, d_rgb = torch.from_numpy(np.ascontiguousarray(xyz)).to(cuda_device), torch.from_numpy(np.ascontiguousarray(rgb)).to(cuda_device)
    line_off, text, status = lio.text_encode_device(d_xyz, d_rgb, fmt)
    off = line_off.cpu().numpy()
    want_off = np.concatenate([[0], np.cumsum([len(ln) for ln in lines])])
    assert int(status.item()) == 0
    np.testing.assert_array_equal(off, want_off)
    got = text[:int(off[-1])].cpu().numpy().tobytes()
    want = b''.join(lines)
    if got != want:
        bad = next(i for i in range(n) if got[off[i]:off[i + 1]] != lines[i])
        pytest.fail('row %d: device %r, host %r' % (bad, got[off[bad]:off[bad + 1]], lines[bad]))
    if n == 4099:                                                # a workgroup's run starts at every byte alignment
        assert set(int(o) % 4 for o in off[:-1:256]) == {0, 1, 2, 3}, sorted(set(int(o) % 4 for o in off[:-1:256]))
    body = lio.encode_points_device(xyz, rgb, [0, n], fmt, device=cuda_device)[0]
    assert bytes(body) == want


def test_strided_rows(cuda_device, crafted):
    """xyz as the leading columns of wider rows (ld > 3)."""
    import torch
    rgb, lines = crafted['ply']
    wide = np.zeros((300, 8), dtype=np.float32)
    wide[:, :3] = crafted['xyz'][:300]
    wide[:, 3:] = np.nan
    line_off, text, status = lio.text_encode_device(torch.from_numpy(wide).to(cuda_device), torch.from_numpy(rgb[:300].copy()).to(cuda_device), 'ply')
    assert int(status.item()) == 0
    assert text[:int(line_off[-1].item())].cpu().numpy().tobytes() == b''.join(lines[:300])


@pytest.mark.parametrize('fmt', ['ply', 'pcd'])
def test_three_rooms_in_one_launch(cuda_device, crafted, tmp_path, fmt, capsys):
    import torch
    rgb = crafted[fmt][0]
    sizes, xyz = [1, 300, 1000], crafted['xyz']
    start = np.concatenate([[0], np.cumsum(sizes)])
    n = int(start[-1])
    bodies, files = [], []
    for r in range(3):
        b, f = _host_body(tmp_path, xyz[start[r]:start[r + 1]], rgb[start[r]:start[r + 1]], fmt, 'h%d' % r)
        bodies.append(b)
        files.append(f)
    line_off, text, status = lio.text_encode_device(torch.from_numpy(xyz[:n].copy()).to(cuda_device), torch.from_numpy(rgb[:n].copy()).to(cuda_device), fmt)
    off = line_off.cpu().numpy()
    assert (np.diff(off) >= 0).all() and int(off[-1]) == sum(len(b) for b in bodies) and int(status.item()) == 0
    got = lio.encode_points_device(xyz[:n], rgb[:n], start, fmt, device=cuda_device)
    assert [bytes(g) for g in got] == bodies
    host_out = capsys.readouterr().out
    names = [str(tmp_path / ('d%d.%s' % (r, fmt))) for r in range(3)]
    routes = lio._save_rooms_device(names, [xyz[start[r]:start[r + 1]] for r in range(3)], [rgb[start[r]:start[r + 1]] for r in range(3)], fmt,
                                    cuda_device)
    assert routes == ['device'] * 3
    assert [open(p, 'rb').read() for p in names] == files
    assert capsys.readouterr().out == host_out.replace(str(tmp_path / 'h'), str(tmp_path / 'd'))


def test_refused_rows_go_to_the_host(cuda_device, crafted, tmp_path):
    """A room with a NaN, an inf and a 2^40 coordinate is counted, contributes empty lines and is written by the host function; the other
    rooms of the batch stay on the device."""
    import torch
    rgb = crafted['ply'][0]
    sizes, xyz = [200, 300, 257], crafted['xyz'][:757].copy()
    start = np.concatenate([[0], np.cumsum(sizes)])
    xyz[200 + 5, 0], xyz[200 + 77, 1], xyz[200 + 299, 2] = np.nan, -np.inf, 2.0 ** 40
    d_xyz, d_rgb = torch.from_numpy(xyz).to(cuda_device), torch.from_numpy(rgb[:757].copy()).to(cuda_device)
    line_off, text, status = lio.text_encode_device(d_xyz, d_rgb, 'ply')
    off = line_off.cpu().numpy()
    assert int(status.item()) == 3
    assert sorted(np.nonzero(np.diff(off) == 0)[0].tolist()) == [205, 277, 499]
    rooms_x, rooms_c = [xyz[start[r]:start[r + 1]] for r in range(3)], [rgb[start[r]:start[r + 1]] for r in range(3)]
    names = [str(tmp_path / ('d%d.ply' % r)) for r in range(3)]
    assert lio.save_rooms_ply_device(names, rooms_x, rooms_c, device=cuda_device) == ['device', 'host', 'device']
    for r in range(3):
        _, want = _host_body(tmp_path, rooms_x[r], rooms_c[r], 'ply', 'h%d' % r)
        assert open(names[r], 'rb').read() == want, r
    assert b'nan' in open(names[1], 'rb').read() and b'-inf' in open(names[1], 'rb').read()
    # PCD: a colour of 256 refuses the row (the host shifts Python integers: the packed value is another number)
    pc = crafted['pcd'][0][:757].copy()
    pc[10, 2], pc[700, 0] = 256, -1
    fin = crafted['xyz'][:757]
    _, _, st = lio.text_encode_device(torch.from_numpy(fin.copy()).to(cuda_device), torch.from_numpy(pc).to(cuda_device), 'pcd')
    assert int(st.item()) == 2
    names = [str(tmp_path / ('d%d.pcd' % r)) for r in range(3)]
    routes = lio._save_rooms_device(names, [fin[start[r]:start[r + 1]] for r in range(3)], [pc[start[r]:start[r + 1]] for r in range(3)], 'pcd', cuda_device)
    assert routes == ['host', 'device', 'host']
    for r in range(3):
        _, want = _host_body(tmp_path, fin[start[r]:start[r + 1]], pc[start[r]:start[r + 1]], 'pcd', 'h%d' % r)
        assert open(names[r], 'rb').read() == want, r
    # ... while PLY prints such colours
    _, _, st = lio.text_encode_device(torch.from_numpy(fin.copy()).to(cuda_device), torch.from_numpy(pc).to(cuda_device), 'ply')
    assert int(st.item()) == 0


def test_savePLY_device_on_the_reference_points(cuda_device, tmp_path, capsys):
    pts = np.load(os.path.join(GOLDEN, 'ref_save_points.npy'))
    assert not np.array_equal(pts[:, :3].astype(np.float32), pts[:, :3])          # float64 values no float32 holds: the host route
    assert lio.savePLY_device(str(tmp_path / 'a.ply'), pts) == 'host'
    assert open(tmp_path / 'a.ply').read() == open(os.path.join(GOLDEN, 'ref_savePLY.ply')).read()
    assert lio.savePCD_device(str(tmp_path / 'a.pcd'), pts) == 'host'
    assert open(tmp_path / 'a.pcd').read() == open(os.path.join(GOLDEN, 'ref_savePCD.pcd')).read()
    capsys.readouterr()
    # the same points rounded to float32: the device route, the same file and the same printed line as the host function
    p32 = np.hstack([pts[:, :3].astype(np.float32).astype(np.float64), pts[:, 3:6]])
    for fmt, host, dev in (('ply', lio.savePLY, lio.savePLY_device), ('pcd', lio.savePCD, lio.savePCD_device)):
        host(str(tmp_path / ('h.' + fmt)), p32)
        want_line = capsys.readouterr().out
        assert dev(str(tmp_path / ('d.' + fmt)), p32, device=cuda_device) == 'device'
        assert capsys.readouterr().out == want_line.replace('h.' + fmt, 'd.' + fmt)
        assert open(tmp_path / ('d.' + fmt), 'rb').read() == open(tmp_path / ('h.' + fmt), 'rb').read()
    # colours that are not integral: the host truncates them, the device is not asked
    frac = p32.copy()
    frac[3, 4] += 0.5
    assert lio.savePLY_device(str(tmp_path / 'f.ply'), frac) == 'host'
    lio.savePLY(str(tmp_path / 'fh.ply'), frac)
    assert open(tmp_path / 'f.ply', 'rb').read() == open(tmp_path / 'fh.ply', 'rb').read()


def test_savePCD_device_on_zero_points_writes_nothing(cuda_device, tmp_path, capsys):
    lio.savePCD_device(str(tmp_path / 'none.pcd'), np.zeros((0, 6)))
    assert not os.path.exists(tmp_path / 'none.pcd') and capsys.readouterr().out == ''
    lio.savePLY_device(str(tmp_path / 'none.ply'), np.zeros((0, 6)))                # savePLY writes the header alone
    lio.savePLY(str(tmp_path / 'none_h.ply'), np.zeros((0, 6)))
    assert open(tmp_path / 'none.ply', 'rb').read() == open(tmp_path / 'none_h.ply', 'rb').read()
