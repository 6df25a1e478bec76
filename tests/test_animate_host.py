"""Host: known answers for the NumPy twin of the growth trace and the renderer (tests/animate_ref.py), the camera matrices, the palette
PNG writer and the font -- the twin is what the GPU tests hold the kernels to, so it is pinned here by hand."""
import math

import numpy as np
import pytest

import animate_ref as ar
import step_audit
from learn_region_grow_amd import io as lio
from learn_region_grow_amd import render, synthetic

W, H = 96, 80
EYE = np.array(ar.EYE)
RIGHT = np.cross(-EYE / np.linalg.norm(EYE), [0, 0, 1.0])
RIGHT /= np.linalg.norm(RIGHT)


def covered(vis, w=W, h=H):
    return np.argwhere(vis.reshape(h, w) != ar.EMPTY)


def test_matrices_against_hand_computed_values():
    f = 1.0 / math.tan(math.radians(35.0))
    p = ar.perspective(70.0, 1.2, 1.0, 1000.0)
    want = np.zeros((4, 4))
    want[0, 0], want[1, 1], want[2, 2], want[2, 3], want[3, 2] = f / 1.2, f, -1001.0 / 999.0, -2000.0 / 999.0, -1.0
    np.testing.assert_allclose(p, want, rtol=1e-15, atol=0)
    assert abs(f - 1.4281480067421144) < 1e-15
    # an eye on the -y axis looking at the origin, z up: x stays, z becomes the picture's y, the view runs along -z
    v = ar.look_at((0, -5, 0))
    np.testing.assert_allclose(v, [[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, -5], [0, 0, 0, 1]], atol=1e-15)
    v = ar.look_at(ar.EYE)
    dist = np.linalg.norm(EYE)
    np.testing.assert_allclose(v @ np.append(EYE, 1), [0, 0, 0, 1], atol=1e-12)
    np.testing.assert_allclose(v @ [0, 0, 0, 1], [0, 0, -dist, 1], atol=1e-12)
    np.testing.assert_allclose(v[:3, :3] @ v[:3, :3].T, np.eye(3), atol=1e-14)
    assert v[1, 2] > 0                                                   # z is up in the picture
    # the package makes the same 16 floats, bit for bit, and rounds once
    for w, h, eye in ((W, H, ar.EYE), (1000, 1000, ar.EYE), (128, 64, render.orbit_eye(ar.EYE, 0.3))):
        got, twin = render.camera_matrix(w, h, eye), ar.camera_matrix(w, h, eye)
        assert got.dtype == np.float32 and got.tobytes() == twin.tobytes()
    x, y, z = render.orbit_eye((3.0, 4.0, 2.0), math.pi / 2)
    np.testing.assert_allclose([x, y, z], [-4.0, 3.0, 2.0], atol=1e-12)


def test_one_point_at_the_centre_covers_25_pixels():
    m = ar.camera_matrix(W, H)
    vis = ar.visibility([[0, 0, 0]], m, W, H, 5)
    rows = H - 1 - np.arange(H // 2 - 2, H // 2 + 3)
    want = sorted((int(r), c) for r in rows for c in range(W // 2 - 2, W // 2 + 3))
    assert sorted(map(tuple, covered(vis).tolist())) == want
    assert (vis[vis != ar.EMPTY] & np.uint64(0xFFFFFFFF) == 0).all()
    assert len(covered(ar.visibility([[0, 0, 0]], m, W, H, 1))) == 1
    with pytest.raises(AssertionError):
        ar.visibility([[0, 0, 0]], m, W, H, 4)


def test_depth_order_ties_and_clipping():
    m = ar.camera_matrix(W, H)
    # the nearer point wins whatever its index
    vis = ar.visibility([[0, 0, 0], 0.1 * EYE], m, W, H, 5)
    assert set((vis[vis != ar.EMPTY] & np.uint64(0xFFFFFFFF)).tolist()) == {1} and len(covered(vis)) == 25
    vis = ar.visibility([0.1 * EYE, [0, 0, 0]], m, W, H, 5)
    assert set((vis[vis != ar.EMPTY] & np.uint64(0xFFFFFFFF)).tolist()) == {0}
    # equal depth: the lower index (the first drawn under GL_LESS)
    vis = ar.visibility([[7, 7, 7], [0, 0, 0], [0, 0, 0]], m, W, H, 5)
    assert set((vis[vis != ar.EMPTY] & np.uint64(0xFFFFFFFF)).tolist()) == {1}
    # behind the eye, and nearer than the near plane: nothing
    assert not len(covered(ar.visibility([1.5 * EYE, 0.95 * EYE], m, W, H, 5)))
    assert not len(covered(ar.visibility([[np.nan, 0, 0], [np.inf, 0, 0]], m, W, H, 5)))
    # a splat at the left border loses the columns outside
    dist = np.linalg.norm(EYE)
    f = 1.0 / math.tan(math.radians(35.0))
    t = -0.995 * dist * (W / float(H)) / f                               # ndc.x = -0.995: column floor(0.0025 * 96) = 0
    px = covered(ar.visibility([t * RIGHT], m, W, H, 5))
    assert sorted(set(px[:, 1].tolist())) == [0, 1, 2] and len(px) == 15


def test_width_and_height_are_not_transposed():
    w, h = 96, 40
    m = ar.camera_matrix(w, h)
    dist = np.linalg.norm(EYE)
    f = 1.0 / math.tan(math.radians(35.0))
    t = 0.5 * dist * (w / float(h)) / f                                  # ndc.x = 0.5: column 72 of 96, middle row
    px = covered(ar.visibility([t * RIGHT], m, w, h, 1), w, h)
    assert px.tolist() == [[h - 1 - h // 2, 72]]
    up = np.cross(RIGHT, -EYE / dist)
    px = covered(ar.visibility([0.5 * dist / f * up], m, w, h, 1), w, h)  # ndc.y = 0.5: row 30 from below = image row 9
    assert px.tolist() == [[h - 1 - 30, w // 2]]


def test_shade_and_text():
    font = render.font_table()
    m = ar.camera_matrix(W, H)
    xyz = np.array([[0, 0, 0], 0.1 * EYE + 2.0 * RIGHT, 0.2 * RIGHT], dtype=np.float32)
    uneq = np.array([2, 0, 2])
    vis = ar.visibility(xyz, m, W, H, 3)
    index = np.array([[4, 2, 1], [0, 7, 19]], dtype=np.uint8)           # codes of a step frame, paints of a seg frame
    out = ar.shade(vis, uneq, index, [0, 1], [ar.text_lines([0, 3, 1, 12, 34, 5, 6]), None], W, H, font)
    raw = (vis & np.uint64(0xFFFFFFFF)).reshape(H, W)
    hit = vis.reshape(H, W) != ar.EMPTY
    text = ar.text_mask(ar.text_lines([0, 3, 1, 12, 34, 5, 6]), W, H, font)
    assert text.any() and not text[:, :(10 * H // 1000)].any()
    assert (out[0][text] == ar.WHITE).all()
    assert (out[0][hit & ~text & (raw == 1)] == ar.GREEN).all()          # raw point 1 -> equalised 0 -> code 4: after
    assert (out[0][hit & ~text & (raw != 1)] == ar.GREY).all()           # equalised 2 -> code 1: before only
    assert (out[1][hit & (raw == 1)] == ar.GREY).all() and (out[1][hit & (raw != 1)] == 19).all() and not (out[1] == ar.WHITE).any()
    assert (out[:, ~hit & ~text] == 0).all()
    # neighbour wins over after (the later assignment of :385)
    assert ar.luts()[0][6] == ar.BLUE and ar.luts()[0][5] == ar.GREEN and ar.luts()[0][1] == ar.GREY
    assert np.array_equal(ar.luts(), render.luts())


def test_font_covers_the_five_lines():
    font = render.font_table()
    assert font.shape == (95, 7) and font.max() < 32
    lines = render.text_lines(123, 4567, 890, 12, 3)
    assert lines == ar.text_lines([0, 123, 0, 4567, 890, 12, 3])
    chars = set(''.join(lines)) | set('0123456789')
    for ch in chars - {' '}:
        assert font[ord(ch) - 32].any(), ch
    glyphs = {font[ord(ch) - 32].tobytes() for ch in chars}
    assert len(glyphs) == len(chars)                                     # no two characters share a drawing
    assert max(len(l) for l in render.text_lines(999, 10 ** 7, 10 ** 7, 10 ** 7, 10 ** 7)) <= render.TEXT_LEN
    block = render.text_block([lines, None])
    assert block.shape == (2, 5, render.TEXT_LEN) and bytes(block[0, 1]).rstrip(b'\0').decode() == lines[1] and not block[1].any()
    assert render.text_geometry(1000) == (5, 10, [10, 60, 110, 160, 210]) and render.text_geometry(128) == (1, 1, [1, 7, 14, 20, 26])


def test_write_png_round_trip(tmp_path):
    pal = render.palette()
    assert pal.shape == (24, 3) and pal[0].tolist() == [0, 0, 0] and pal[20].tolist() == [100, 100, 100] and pal[23].tolist() == [255] * 3
    assert np.array_equal(pal[1:20], np.random.RandomState(0).randint(0, 255, (20, 3))[1:20])
    for shape in ((7, 13), (1, 1), (64, 31)):
        index = np.random.RandomState(shape[0]).randint(0, 24, shape).astype(np.uint8)
        index.flat[0] = 23
        path = str(tmp_path / 'f.png')
        lio.write_png(path, index, pal)
        got = lio.read_png(path)
        assert got.dtype == np.uint8 and np.array_equal(got, pal[index])
    data = open(path, 'rb').read()
    assert data[25] == 3 and b'PLTE' in data                             # colour type 3
    with pytest.raises(ValueError):
        lio.write_png(path, np.full((2, 2), 24, np.uint8), pal)


def test_write_png_is_read_by_pil(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    pal = render.palette()
    index = np.random.RandomState(5).randint(0, 24, (33, 20)).astype(np.uint8)
    path = str(tmp_path / 'g.png')
    lio.write_png(path, index, pal)
    assert np.array_equal(np.asarray(Image.open(path).convert('RGB')), pal[index])


@pytest.fixture(scope='module')
def oracle_trace():
    from oracle import lrgnet_ref
    weights = synthetic.make_synthetic_weights(**ar.WEIGHT_KW)
    room, _, uneq = ar.trace_room()
    res, recs = step_audit.oracle_run(room, ar.TRACE_SEEDS[0], policy='net', net_fn=lambda xi, xn: lrgnet_ref.forward(weights, xi, xn, lite=0))
    return room, uneq, res, recs, ar.trace_from_records(room['points'], recs, res, uneq)


def test_trace_from_records_invariants(oracle_trace):
    room, uneq, res, recs, (headers, codes, paints) = oracle_trace
    n = len(room['points'])
    assert len(headers) == len(recs) == sum(r['steps'] for r in res.regions) > 0
    before, nb, after = (codes & 1).astype(bool), (codes >> 1 & 1).astype(bool), (codes >> 2 & 1).astype(bool)
    assert not (before & nb).any() and nb.any(axis=1).all() and before.any(axis=1).all()
    mult = np.bincount(uneq, minlength=n)
    assert mult.max() > 1
    j, cid = 0, 1
    for r in res.regions:
        for s in range(r['steps']):
            assert headers[j, 0] == r['seed'] and headers[j, 1] == s + 1 and headers[j, 2] == cid
            assert headers[j, 3] == mult[before[j]].sum() and headers[j, 5] == mult[after[j] & ~before[j]].sum()
            if s == 0:
                assert before[j].sum() == 1 and before[j, r['seed']]
            else:
                assert np.array_equal(before[j], after[j - 1])
            j += 1
        if r['steps']:
            assert after[j - 1].sum() == r['points']                     # the last `after` of a region is the region
            if r['labeled']:
                assert np.array_equal(after[j - 1], res.cluster_label == cid)
                assert (paints[j - 1][after[j - 1]] == (cid - 1) % 19 + 1).all()
        cid += 1 if r['labeled'] else 0
    assert j == len(headers)
    assert ((paints[1:] != 0) | (paints[:-1] == 0)).all()               # paint is never taken back
    assert ar.trace_conditions(res) == (True, True, True)              # (the room was chosen for them)
