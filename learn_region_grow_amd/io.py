"""File formats either side of the region-grow path, with the reference's function names and behaviour:

``loadFromH5``  learn_region_grow_util.py:11-31   rooms out of an HDF5 file ('points' [N,F+2], 'count_room' [R])
``saveToH5``    tools/generate_synthetic_rooms.py:111-115 (what the reference's staging tools write)
``savePLY``     learn_region_grow_util.py:57-73   ASCII PLY, "%f %f %f %d %d %d" per vertex
``savePCD``     learn_region_grow_util.py:33-55   ASCII PCD v0.7 with packed rgb
``label_colors`` test_region_grow.py:368-371      the colour table of the result clouds
``read_png``    stage_semantic_kitti.py:103       what imageio.imread gives for the camera images, from zlib and NumPy alone
``write_png``   animate_region_growing.py:402,409 image.save(..., 'PNG') of a frame, as a palette image

HDF5 goes through ``h5lite`` (h5py is not installed here); weights through ``checkpoint``.
"""
import struct
import zlib

import numpy as np

from . import h5lite


def loadFromH5(filename, load_labels=True):
    """Rooms of an HDF5 room file: 'points' holds every room's rows back to back, 'count_room' how many belong to each room.
    Returns the per-room arrays, or (features, object ids, class ids) per room with the last two columns split off."""
    f = h5lite.File(filename)
    rows, counts = f['points'].read(), f['count_room'].read()
    rooms = np.split(rows, np.cumsum(counts)[:-1]) if len(counts) else []
    if not load_labels:
        return rooms
    return ([r[:, :-2] for r in rooms], [r[:, -2].astype(int) for r in rooms], [r[:, -1].astype(int) for r in rooms])


def saveToH5(filename, rooms):
    """rooms: list of [n_i, F+2] arrays (features, object id, class id) -> 'points' float32 + 'count_room' int32."""
    count = np.array([len(r) for r in rooms], dtype=np.int32)
    pts = np.vstack(rooms).astype(np.float32) if len(rooms) else np.zeros((0, 8), np.float32)
    h5lite.write_file(filename, {'points': pts, 'count_room': count})


def savePLY(filename, points):
    with open(filename, 'w') as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % len(points))
        for p in points:
            f.write("%f %f %f %d %d %d\n" % (p[0], p[1], p[2], p[3], p[4], p[5]))
    print('Saved to %s: (%d points)' % (filename, len(points)))


def savePCD(filename, points):
    if len(points) == 0:
        return
    n = len(points)
    with open(filename, 'w') as f:
        f.write("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F I\n"
                "COUNT 1 1 1 1\nWIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA ascii\n" % (n, n))
        for p in points:
            rgb = (int(p[3]) << 16) | (int(p[4]) << 8) | int(p[5])
            f.write("%f %f %f %d\n" % (p[0], p[1], p[2], rgb))
    print('Saved %d points to %s' % (n, filename))


def label_colors(n_labels):
    """Colour per cluster id as the reference draws them (test_region_grow.py:368-370): RandomState(0), id 0 grey."""
    obj_color = np.random.RandomState(0).randint(0, 255, (n_labels, 3))
    obj_color[0] = [100, 100, 100]
    return obj_color


def _png_unfilter(raw, height, stride, bpp):
    """The scanlines of an inflated PNG stream without their filters (PNG 1.2, section 6): [height, stride] uint8."""
    if len(raw) != height * (stride + 1):
        raise ValueError('PNG: %d bytes of image data, %d expected' % (len(raw), height * (stride + 1)))
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(height, stride + 1)
    out = np.zeros((height + 1, stride), dtype=np.uint8)                  # row 0: the zeros above the first scanline
    for r in range(height):
        kind, line, up = int(rows[r, 0]), rows[r, 1:], out[r]
        cur = out[r + 1]
        if kind == 0:
            cur[:] = line
        elif kind == 1:                                                    # Sub: a running sum per byte lane of the pixel
            for lane in range(bpp):
                cur[lane::bpp] = np.cumsum(line[lane::bpp], dtype=np.uint64).astype(np.uint8)
        elif kind == 2:                                                    # Up
            cur[:] = line + up
        elif kind in (3, 4):                                               # Average, Paeth: each byte needs the one bpp to its left
            l, u, o = line.tolist(), up.tolist(), [0] * stride
            for i in range(stride):
                a = o[i - bpp] if i >= bpp else 0
                if kind == 3:
                    pred = (a + u[i]) >> 1
                else:
                    c = u[i - bpp] if i >= bpp else 0
                    pa, pb, pc = abs(u[i] - c), abs(a - c), abs(a + u[i] - 2 * c)
                    pred = a if pa <= pb and pa <= pc else (u[i] if pb <= pc else c)
                o[i] = (l[i] + pred) & 255
            cur[:] = o
        else:
            raise ValueError('PNG: unknown filter type %d in row %d' % (kind, r))
    return out[1:]


def read_png(filename):
    """An 8-bit, non-interlaced grey, RGB, RGBA or palette PNG as uint8 [H, W, 3] (grey repeated, alpha dropped, palette entries looked up).
    Any other PNG is an error."""
    with open(filename, 'rb') as f:
        data = f.read()
    if data[:8] != b'\x89PNG\r\n\x1a\n':
        raise ValueError('%s is not a PNG file' % filename)
    pos, header, idat, ended, plte = 8, None, [], False, None
    while pos + 8 <= len(data) and not ended:
        length, tag = struct.unpack('>I4s', data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + length]
        if len(body) != length or pos + 12 + length > len(data):
            raise ValueError('%s: truncated %s chunk' % (filename, tag.decode('latin-1')))
        if struct.unpack('>I', data[pos + 8 + length:pos + 12 + length])[0] != (zlib.crc32(tag + body) & 0xFFFFFFFF):
            raise ValueError('%s: bad CRC in %s chunk' % (filename, tag.decode('latin-1')))
        if tag == b'IHDR':
            header = struct.unpack('>IIBBBBB', body)
        elif tag == b'PLTE':
            plte = body
        elif tag == b'IDAT':
            idat.append(body)
        elif tag == b'IEND':
            ended = True
        pos += 12 + length
    if header is None or not idat or not ended:
        raise ValueError('%s: IHDR, IDAT or IEND missing' % filename)
    width, height, depth, colour, compression, filtering, interlace = header
    if depth != 8 or colour not in (0, 2, 3, 6) or compression != 0 or filtering != 0 or interlace != 0 or width < 1 or height < 1:
        raise ValueError('%s: only 8-bit non-interlaced grey / RGB / RGBA / palette PNGs are read (bit depth %d, colour type %d, interlace %d)' %
                         (filename, depth, colour, interlace))
    bpp = {0: 1, 2: 3, 3: 1, 6: 4}[colour]
    if colour == 3 and (plte is None or len(plte) % 3 or not 3 <= len(plte) <= 768):
        raise ValueError('%s: a palette image without a valid PLTE chunk' % filename)
    try:
        raw = zlib.decompress(b''.join(idat))
    except zlib.error as e:
        raise ValueError('%s: %s' % (filename, e))
    px = _png_unfilter(raw, height, width * bpp, bpp).reshape(height, width, bpp)
    if colour == 3:
        table = np.frombuffer(plte, dtype=np.uint8).reshape(-1, 3)
        if int(px.max()) >= len(table):
            raise ValueError('%s: pixel value %d outside the palette of %d entries' % (filename, int(px.max()), len(table)))
        return np.ascontiguousarray(table[px[:, :, 0]])
    return np.ascontiguousarray(np.repeat(px, 3, axis=2) if bpp == 1 else px[:, :, :3])


def _png_chunk(tag, body):
    return struct.pack('>I', len(body)) + tag + body + struct.pack('>I', zlib.crc32(tag + body) & 0xFFFFFFFF)


def encode_png(index, palette, level=1):
    """The bytes of a palette PNG (colour type 3, 8 bits, every row under filter 0, one IDAT): index [H, W] uint8, palette [P <= 256, 3]."""
    index, palette = np.ascontiguousarray(index, dtype=np.uint8), np.ascontiguousarray(palette, dtype=np.uint8)
    if index.ndim != 2 or index.size == 0 or palette.ndim != 2 or palette.shape[1] != 3 or not 1 <= len(palette) <= 256:
        raise ValueError('write_png: index [H, W] and palette [P <= 256, 3] expected, got %s and %s' % (index.shape, palette.shape))
    height, width = index.shape
    rows = np.zeros((height, width + 1), dtype=np.uint8)          # column 0: filter type 0
    rows[:, 1:] = index
    return (b'\x89PNG\r\n\x1a\n' + _png_chunk(b'IHDR', struct.pack('>IIBBBBB', width, height, 8, 3, 0, 0, 0)) + _png_chunk(b'PLTE', palette.tobytes()) +
            _png_chunk(b'IDAT', zlib.compress(rows.tobytes(), level)) + _png_chunk(b'IEND', b''))


def write_png(filename, index, palette, level=1):
    """A frame as a palette PNG: what read_png (or any viewer) turns back into palette[index].  A pixel value outside the palette is an error."""
    index = np.asarray(index)
    if index.size and int(index.max()) >= len(palette):
        raise ValueError('write_png: pixel value %d outside the palette of %d entries' % (int(index.max()), len(palette)))
    with open(filename, 'wb') as f:
        f.write(encode_png(index, palette, level))


# ---- vertex lines encoded on the device (lrg_text_encode, csrc/lrg_text.hip) ----------------------------------------
# The host functions above stay the authority: what follows writes the same bytes and prints the same lines, and hands every room the
# device refuses (a non-finite coordinate, |x| >= 2^40, a PCD colour outside 0 .. 255), and every array that is not float32 / integral,
# back to them.

TEXT_FORMATS = {'ply': 0, 'pcd': 1}


def _ply_header(n):
    return ("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % n)


def _pcd_header(n):
    return ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F I\n"
            "COUNT 1 1 1 1\nWIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA ascii\n" % (n, n))


def text_rows_per_call():
    """The most rows one lrg_text_encode call takes: the byte offsets are int32 and the text is sized from the bound rows * LRG_TEXT_MAX_LINE."""
    from . import _lib
    return ((1 << 31) - 1) // _lib.LRG_TEXT_MAX_LINE


def text_encode_device(xyz, rgb, format='ply'):
    """The lines of xyz [n, >= 3] float32 (rows may be strided) and rgb [n, 3] int32, device tensors, enqueued on the current stream of their
    device: (line_off [n + 1] int32, text uint8, status [1] int32) on the device, nothing synchronised.  Line i is
    text[line_off[i]:line_off[i + 1]], empty for a refused row; status counts the refused rows."""
    import torch
    from . import _lib
    from .lrgnet import _ptr, _stream_ptr
    if format not in TEXT_FORMATS:
        raise ValueError("format must be 'ply' or 'pcd', not %r" % (format,))
    n = int(xyz.shape[0])
    if not (xyz.is_cuda and rgb.is_cuda and xyz.dtype == torch.float32 and rgb.dtype == torch.int32 and xyz.dim() == 2 and xyz.shape[1] >= 3 and
            tuple(rgb.shape) == (n, 3)):
        raise ValueError('text_encode_device: xyz [n, >= 3] float32 and rgb [n, 3] int32 on the device expected')
    if n > text_rows_per_call():
        raise ValueError('text_encode_device: %d rows in one call, at most %d (split the batch at room boundaries)' % (n, text_rows_per_call()))
    if n and (xyz.stride(1) != 1 or xyz.stride(0) < 3):
        xyz = xyz[:, :3].contiguous()
    rgb = rgb.contiguous()
    lib, dev = _lib.load(), xyz.device
    with torch.cuda.device(dev):
        ws = torch.empty(lib.lrg_text_workspace_bytes(n), dtype=torch.uint8, device=dev)
        line_off = torch.empty(n + 1, dtype=torch.int32, device=dev)
        text = torch.empty(max(16, n * _lib.LRG_TEXT_MAX_LINE), dtype=torch.uint8, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.check(lib.lrg_text_encode(_ptr(xyz), int(xyz.stride(0)) if n else 3, _ptr(rgb), n, TEXT_FORMATS[format], _ptr(ws), ws.numel(),
                                       _ptr(line_off), _ptr(text), text.numel(), _ptr(status), _stream_ptr(dev)), 'lrg_text_encode')
    return line_off, text, status


def _encode_call(xyz, rgb, starts, format):
    """One launch over the rooms starts[0] .. starts[-1] of device tensors: their bodies as memoryviews into one pinned download, None for a
    room with a refused row.  One synchronisation before the download."""
    import torch
    dev = xyz.device
    a, b = int(starts[0]), int(starts[-1])
    line_off, text, status = text_encode_device(xyz[a:b], rgb[a:b], format)
    with torch.cuda.device(dev):
        at = torch.as_tensor(np.asarray(starts, dtype=np.int64) - a, device=dev)
        head = torch.cat([line_off.index_select(0, at), status]).to('cpu', non_blocking=False).numpy()      # the offsets and the status together
        offs, refused = head[:-1], int(head[-1])
        total = int(offs[-1])
        host = torch.empty(max(total, 1), dtype=torch.uint8).pin_memory()
        host[:total].copy_(text[:total], non_blocking=True)
        bad = None
        if refused:
            gone = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), (line_off[1:] == line_off[:-1]).cumsum(0)])
            bad = gone.index_select(0, at).cpu().numpy()
        torch.cuda.current_stream(dev).synchronize()
    view = memoryview(host.numpy())
    out = []
    for r in range(len(starts) - 1):
        if bad is not None and bad[r + 1] > bad[r]:
            out.append(None)
        else:
            out.append(view[int(offs[r]):int(offs[r + 1])])
    return out


def encode_points_device(xyz, rgb, raw_start, format='ply', device=None):
    """The file bodies of the rooms raw_start[r] .. raw_start[r + 1] of xyz [n, >= 3] float32 and rgb [n, 3] int32 (NumPy arrays or device
    tensors): one memoryview per room into a pinned download, or None for a room the device refused (a row with a non-finite coordinate,
    |x| >= 2^40 or, for 'pcd', a colour outside 0 .. 255) or that is too large for one call: such a room is the host function's.  All rooms
    go through one launch (more only where rows * LRG_TEXT_MAX_LINE would pass 2^31), split at room boundaries."""
    import torch
    raw_start = [int(v) for v in raw_start]
    if len(raw_start) < 1 or raw_start[0] != 0 or any(b < a for a, b in zip(raw_start, raw_start[1:])) or raw_start[-1] != len(xyz):
        raise ValueError('encode_points_device: raw_start must rise from 0 to the number of rows')
    if not torch.is_tensor(xyz):
        dev = torch.device(device if device is not None else 'cuda')
        xyz = torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.float32)).to(dev)
    dev = xyz.device
    if not torch.is_tensor(rgb):
        rgb = torch.from_numpy(np.ascontiguousarray(rgb, dtype=np.int32))
    rgb = rgb.to(dev)
    cap, out, r, R = text_rows_per_call(), [], 0, len(raw_start) - 1
    while r < R:
        if raw_start[r + 1] - raw_start[r] > cap:
            out.append(None)
            r += 1
            continue
        e = r + 1
        while e < R and raw_start[e + 1] - raw_start[r] <= cap:
            e += 1
        out.extend(_encode_call(xyz, rgb, raw_start[r:e + 1], format))
        r = e
    return out


def _save_rooms_device(filenames, xyz_rooms, rgb_rooms, format, device=None):
    import torch
    if not (len(filenames) == len(xyz_rooms) == len(rgb_rooms)):
        raise ValueError('one file name, one xyz array and one rgb array per room expected')
    if not filenames:
        return []
    start = np.concatenate([[0], np.cumsum([len(x) for x in xyz_rooms])])
    if torch.is_tensor(xyz_rooms[0]):
        xyz = torch.cat([x[:, :3] for x in xyz_rooms]) if len(xyz_rooms) > 1 else xyz_rooms[0]
        rgb = torch.cat(list(rgb_rooms)) if len(rgb_rooms) > 1 else rgb_rooms[0]
    else:
        xyz = np.concatenate([np.asarray(x, dtype=np.float32)[:, :3] for x in xyz_rooms])
        rgb = np.concatenate([np.asarray(c, dtype=np.int32) for c in rgb_rooms])
    bodies = encode_points_device(xyz, rgb, start, format, device)
    routes = []
    for name, body, x, c in zip(filenames, bodies, xyz_rooms, rgb_rooms):
        n = len(x)
        if body is None:
            x, c = (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)), (c.cpu().numpy() if torch.is_tensor(c) else np.asarray(c))
            (savePLY if format == 'ply' else savePCD)(name, np.hstack([x[:, :3].astype(np.float64), c.astype(np.float64)]))
            routes.append('host')
            continue
        routes.append('device')
        if format == 'pcd' and n == 0:
            continue
        with open(name, 'wb') as f:
            f.write((_ply_header(n) if format == 'ply' else _pcd_header(n)).encode('ascii'))
            f.write(body)
        print('Saved to %s: (%d points)' % (name, n) if format == 'ply' else 'Saved %d points to %s' % (n, name))
    return routes


def save_rooms_ply_device(filenames, xyz_rooms, rgb_rooms, device=None):
    """savePLY of several rooms through one launch: xyz_rooms[r] [n_r, >= 3] float32 and rgb_rooms[r] [n_r, 3] int32, NumPy arrays or device
    tensors.  The same files and the same printed lines as savePLY; returns 'device' or 'host' per room, the route it took (a room with a
    refused row is written by savePLY itself)."""
    return _save_rooms_device(filenames, xyz_rooms, rgb_rooms, 'ply', device)


def _device_rows(points):
    """xyz float32 and rgb int32 of a points array, or None where the device would not print what the host prints: a coordinate that is
    not a float32 value, a colour that is not an int32 value (the host's %d truncates, its %f prints the double)."""
    points = np.asarray(points)
    if points.ndim != 2 or points.shape[1] < 6 or points.dtype.kind not in 'fiu':
        return None
    a = points[:, :6].astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        xyz, rgb = a[:, :3].astype(np.float32), a[:, 3:6].astype(np.int32)
        same = np.array_equal(np.hstack([xyz, rgb]), a)           # one comparison; a NaN differs from itself and goes to the host too
    return (xyz, rgb) if same else None


def savePLY_device(filename, points, device=None):
    """savePLY with the vertex lines encoded on the device: the same file, the same printed line.  Returns the route taken."""
    rows = _device_rows(points) if len(points) else None
    if rows is None:
        savePLY(filename, points)
        return 'host'
    return _save_rooms_device([filename], [rows[0]], [rows[1]], 'ply', device)[0]


def savePCD_device(filename, points, device=None):
    """savePCD with the vertex lines encoded on the device: the same file, the same printed line, nothing written for zero points."""
    if len(points) == 0:
        return 'host'
    rows = _device_rows(points)
    if rows is None:
        savePCD(filename, points)
        return 'host'
    return _save_rooms_device([filename], [rows[0]], [rows[1]], 'pcd', device)[0]
