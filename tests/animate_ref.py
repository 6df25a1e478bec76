"""NumPy twin of the growth trace and the renderer (learn_region_grow_amd.trace / render, csrc/lrg_trace.hip): what the GPU tests compare
bit for bit, and what test_animate_host.py pins with known answers.  Nothing here imports the package's renderer: the matrices, the
rasteriser, the shading, the text geometry and the trace are restated from animate_region_growing.py and DESIGN 3.21.
"""
import math

import numpy as np

from oracle import grow_ref

EYE = (9.42495995258856, 9.381724865127635, 4.651620026309769)
GREY, GREEN, BLUE, WHITE = 20, 21, 22, 23
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def look_at(eye, centre=(0, 0, 0), up=(0, 0, 1)):
    eye, centre, up = np.array(eye, float), np.array(centre, float), np.array(up, float)
    f = (centre - eye) / np.linalg.norm(centre - eye)
    s = np.cross(f, up)
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    return np.array([[s[0], s[1], s[2], -s.dot(eye)], [u[0], u[1], u[2], -u.dot(eye)], [-f[0], -f[1], -f[2], f.dot(eye)], [0, 0, 0, 1.0]])


def perspective(fovy, aspect, zn, zf):
    f = 1.0 / math.tan(fovy * math.pi / 360.0)
    return np.array([[f / aspect, 0, 0, 0], [0, f, 0, 0], [0, 0, (zf + zn) / (zn - zf), 2 * zf * zn / (zn - zf)], [0, 0, -1.0, 0]])


def camera_matrix(W, H, eye=EYE, centre=(0, 0, 0)):
    return (perspective(70.0, W / float(H), 1.0, 1000.0) @ look_at(eye, centre)).astype(np.float32)


def project(xyz, mat):
    """-> (kept raw indices, ix, iy, depth float32) in float32 arithmetic, one rounding per operation."""
    p = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    m = np.asarray(mat, dtype=np.float32).reshape(4, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all='ignore'):
        c = [((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(4)]
        w = c[3]
        keep = w > 0
        for q in c[:3]:
            keep &= (-w <= q) & (q <= w)
        idx = np.flatnonzero(keep)
        w = w[idx]
        nx, ny, nz = c[0][idx] / w, c[1][idx] / w, c[2][idx] / w
    return idx, nx, ny, nz


def visibility(xyz, mat, W, H, size):
    assert size % 2 == 1
    idx, nx, ny, nz = project(xyz, mat)
    half = np.float32(0.5)
    xw, yw = (nx * half + half) * np.float32(W), (ny * half + half) * np.float32(H)
    depth = (nz * half + half).astype(np.float32)
    assert xw.dtype == np.float32 and depth.dtype == np.float32
    with np.errstate(invalid='ignore'):
        ok = (xw >= 0) & (xw <= np.float32(W)) & (yw >= 0) & (yw <= np.float32(H))      # (true of every finite point; a NaN from inf / inf stays out)
    idx, xw, yw, depth = idx[ok], xw[ok], yw[ok], depth[ok]
    ix, iy = np.floor(xw).astype(np.int64), np.floor(yw).astype(np.int64)
    key = (depth.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
    vis = np.full(H * W, EMPTY, dtype=np.uint64)
    h = (size - 1) // 2
    for dy in range(-h, h + 1):
        for dx in range(-h, h + 1):
            px, py = ix + dx, iy + dy
            ok = (px >= 0) & (px < W) & (py >= 0) & (py < H)
            np.minimum.at(vis, ((H - 1 - py[ok]) * W + px[ok]), key[ok])
    return vis


def luts():
    code = np.arange(256)
    seg = np.full(256, GREY)
    seg[1:20] = np.arange(1, 20)
    return np.stack([np.where(code & 2, BLUE, np.where(code & 4, GREEN, GREY)), seg]).astype(np.uint8)


def text_mask(lines, W, H, font, font_first=32, text_len=40):
    """[H, W] bool: the strokes of up to five lines."""
    scale, x0 = max(1, 40 * H // 8000), 10 * H // 1000
    out = np.zeros((H, W), dtype=bool)
    for k, line in enumerate(lines):
        y0 = (10 + 50 * k) * H // 1000
        for ci, ch in enumerate(line[:text_len]):
            g = ord(ch) - font_first
            if not 0 <= g < len(font):
                continue
            for r in range(7):
                for c in range(5):
                    if font[g][r] >> (4 - c) & 1:
                        ya, xa = y0 + r * scale, x0 + (6 * ci + c) * scale
                        out[ya:ya + scale, xa:xa + scale] = True      # (slices clip at the window's edge)
    return out


def shade(vis, uneq, index, frame_lut, texts, W, H, font):
    """-> [T, H, W] uint8.  index [T, >= n]; texts: per frame None or five strings."""
    vis = np.asarray(vis, dtype=np.uint64)
    hit = vis != EMPTY
    raw = (vis & np.uint64(0xFFFFFFFF)).astype(np.int64)
    eq = np.where(hit, np.asarray(uneq)[np.where(hit, raw, 0)], 0)
    table = luts()
    out = np.zeros((len(index), H, W), dtype=np.uint8)
    for t in range(len(index)):
        out[t] = np.where(hit, table[frame_lut[t]][np.asarray(index[t])[eq]], 0).reshape(H, W)
        if texts is not None and texts[t]:
            out[t][text_mask(texts[t], W, H, font)] = WHITE
    return out


def text_lines(h):
    return ['Step %d' % h[1], 'Inlier Set: %d points' % h[3], 'Neighbor Set: %d points' % h[4], 'Add: %d points' % h[5], 'Remove: %d points' % h[6]]


# The room of the trace tests and the counter-stream seeds to try on it, chosen on the CPU (oracle/lrgnet_ref under the synthetic weights of
# test_gpu_grow.py): under each of these seeds the oracle run holds a region ended by 'stuck', one ended after steps by 'noexpand' or
# 'noneighbor', and a zero-step 'noneighbor' seed logged directly behind a finished region (trace_conditions).  1 506 equalised points
# (not a multiple of 4) out of 4 065 raw ones (not a multiple of 64).
TRACE_ROOM = dict(n_raw=1100, seed=505, n_furniture=2, room_id=3)
TRACE_SEEDS = (11, 14, 16, 24)
WEIGHT_KW = dict(seed=0, gain=2.0, bias_std=0.2, add_bias_shift=0.0, rmv_bias_shift=-3.0)


def trace_room():
    """-> (room dict for RegionGrower.load_rooms, raw xyz [M, 3], unequalized_idx [M])."""
    from learn_region_grow_amd import preprocess, synthetic
    raw = synthetic.area5_shaped_room(TRACE_ROOM['n_raw'], TRACE_ROOM['seed'], n_furniture=TRACE_ROOM['n_furniture']).astype(np.float32)
    p = preprocess.preprocess_room(raw[:, :6], raw[:, 6].astype(int), raw[:, 7].astype(int))
    return dict(points=p['points'], obj_id=p['obj_id'], order=p['order'], room_id=TRACE_ROOM['room_id']), raw[:, :3].copy(), p['unequalized_idx']


def trace_conditions(result):
    """(a region ended by 'stuck', one ended after steps by 'noexpand' / 'noneighbor', a zero-step 'noneighbor' seed directly behind a finished region)."""
    regs = result.regions
    return (any(r['reason'] == 'stuck' for r in regs),
            any(r['steps'] > 0 and r['reason'] in ('noexpand', 'noneighbor') for r in regs),
            any(a['steps'] > 0 and b['steps'] == 0 and b['reason'] == 'noneighbor' for a, b in zip(regs, regs[1:])))


def _mask(rec, which):
    return np.unpackbits(rec[which], count=rec['n']).astype(bool)


def trace_from_records(points, recs, result, uneq=None, resolution=0.1):
    """recs: the slim hook records of step_audit.oracle_run in evaluation order ({(seed, restart, step): record}), result: its GrowResult.
    -> headers [T, 7] (seed, 1-based step, cluster id, inlier, neighbour, add, remove), codes [T, n], paints [T, n]."""
    n = len(points)
    mult = np.bincount(np.arange(n) if uneq is None else np.asarray(uneq), minlength=n)
    vox = grow_ref.voxelize(np.asarray(points)[:, :3], resolution)
    regions = result.regions
    where = {r['seed']: k for k, r in enumerate(regions)}
    cid_of, cid = {}, 1
    for r in regions:
        cid_of[r['seed']] = cid
        cid += 1 if r['labeled'] else 0
    keys = list(recs)
    headers, codes, paints = np.zeros((len(keys), 7), np.int64), np.zeros((len(keys), n), np.uint8), np.zeros((len(keys), n), np.uint8)
    paint = np.zeros(n, dtype=np.uint8)
    for j, key in enumerate(keys):
        rec = recs[key]
        seed, restart, step = key
        assert restart == 0
        before, visited = _mask(rec, 'mask_bits'), _mask(rec, 'visited_bits')
        box = np.all(vox >= rec['min_dims'] - 1, axis=1) & np.all(vox <= rec['max_dims'] + 1, axis=1)
        neighbour = box & ~before & ~visited
        nxt = keys[j + 1] if j + 1 < len(keys) else None
        if nxt is not None and nxt[0] == seed:
            assert nxt[2] == step + 1
            after = _mask(recs[nxt], 'mask_bits')
        else:
            # the region stopped: what became visited since, less the seeds of the zero-step regions logged behind it
            later = _mask(recs[nxt], 'visited_bits') if nxt is not None else np.ones(n, bool)
            after = later & ~visited
            k = where[seed] + 1
            while k < len(regions) and (nxt is None or regions[k]['seed'] != nxt[0]):
                assert regions[k]['steps'] == 0 and regions[k]['reason'] == 'noneighbor' and regions[k]['points'] == 1
                after[regions[k]['seed']] = False
                k += 1
        c = cid_of[seed]
        paint[after] = (c - 1) % 19 + 1
        codes[j] = before.astype(np.uint8) | (neighbour.astype(np.uint8) << 1) | (after.astype(np.uint8) << 2)
        paints[j] = paint
        headers[j] = [seed, step + 1, c, mult[before].sum(), mult[neighbour].sum(), mult[after & ~before].sum(), mult[before & ~after].sum()]
    return headers, codes, paints
