"""Frames of animate_region_growing.py without OpenGL: the raw points of a room are rasterised ONCE per camera into a visibility buffer
(lrg_render_visibility: GL_POINTS squares under the depth test, :165-182), and every frame is a look-up through it
(lrg_render_shade: result_points[:,3:6] = colour[unequalized_idx], :387,:404) with the five text lines of :397-401 blitted from a
bitmap font.  Frames are palette-index images (io.write_png stores them as they are).

Palette: 0 background, 1 .. 19 instance_color_id[1 .. 19] (:35), 20 the grey (100, 100, 100), 21 green, 22 blue (:382-385), 23 white.
"""
import ctypes
import math

import numpy as np

CAMERA = (9.42495995258856, 9.381724865127635, 4.651620026309769)      # :43-45
LOOK_AT = (0.0, 0.0, 0.0)                                              # :46-48
UP = (0.0, 0.0, 1.0)                                                   # :49-51
FOV, Z_NEAR, Z_FAR = 70.0, 1.0, 1000.0                                 # :56,:255
GREY, GREEN, BLUE, WHITE = 20, 21, 22, 23
TEXT_LINES, TEXT_LEN = 5, 40
LUT_STEP, LUT_SEG = 0, 1


def palette():
    """[24, 3] uint8."""
    pal = np.zeros((24, 3), dtype=np.uint8)
    pal[1:20] = np.random.RandomState(0).randint(0, 255, (20, 3))[1:20]      # color_sample_state, :34-35
    pal[GREY], pal[GREEN], pal[BLUE], pal[WHITE] = (100, 100, 100), (0, 255, 0), (0, 0, 255), (255, 255, 255)
    return pal


def luts():
    """[2, 256] uint8: code byte -> palette entry of a step frame (:382-385, the later assignment wins: neighbour over current), paint byte -> palette
    entry of a seg frame (:162,:403: unpainted points are grey)."""
    t = np.full((2, 256), GREY, dtype=np.uint8)
    code = np.arange(256)
    t[LUT_STEP] = np.where(code & 2, BLUE, np.where(code & 4, GREEN, GREY))
    t[LUT_SEG, 1:20] = np.arange(1, 20)
    return t


def look_at(eye, centre, up):
    """gluLookAt (:169) as a float64 4 x 4 matrix acting on column vectors."""
    eye, centre, up = (np.asarray(v, dtype=np.float64) for v in (eye, centre, up))
    f = centre - eye
    f = f / np.linalg.norm(f)
    s = np.cross(f, up)
    s = s / np.linalg.norm(s)
    u = np.cross(s, f)
    m = np.eye(4)
    m[0, :3], m[1, :3], m[2, :3] = s, u, -f
    m[0, 3], m[1, 3], m[2, 3] = -s.dot(eye), -u.dot(eye), f.dot(eye)      # (glTranslated(-eye) behind the rotation)
    return m


def perspective(fovy_deg, aspect, z_near, z_far):
    """gluPerspective (:255)."""
    f = 1.0 / math.tan(math.radians(fovy_deg) / 2.0)
    m = np.zeros((4, 4))
    m[0, 0], m[1, 1] = f / aspect, f
    m[2, 2], m[2, 3] = (z_far + z_near) / (z_near - z_far), 2.0 * z_far * z_near / (z_near - z_far)
    m[3, 2] = -1.0
    return m


def orbit_eye(eye, angle):
    """The eye turned by `angle` radians about the z axis: the rotation the reference has commented out at :377-381."""
    rho, theta = math.hypot(eye[0], eye[1]), math.atan2(eye[1], eye[0]) + angle
    return (rho * math.cos(theta), rho * math.sin(theta), eye[2])


def camera_matrix(W, H, eye=CAMERA, centre=LOOK_AT, up=UP):
    """projection x view, made in float64 and rounded once: the 16 floats lrg_render_visibility takes."""
    return (perspective(FOV, float(W) / float(H), Z_NEAR, Z_FAR) @ look_at(eye, centre, up)).astype(np.float32)


def text_lines(step, inlier, neighbor, add, remove):
    """:397-401."""
    return ['Step %d' % step, 'Inlier Set: %d points' % inlier, 'Neighbor Set: %d points' % neighbor, 'Add: %d points' % add, 'Remove: %d points' % remove]


def text_block(frames):
    """frames: per frame None or five strings -> [T, 5, TEXT_LEN] uint8, 0 where nothing is drawn."""
    out = np.zeros((len(frames), TEXT_LINES, TEXT_LEN), dtype=np.uint8)
    for t, lines in enumerate(frames):
        for k, line in enumerate(lines or ()):
            b = line.encode('ascii')[:TEXT_LEN]
            out[t, k, :len(b)] = np.frombuffer(b, dtype=np.uint8)
    return out


# A 5 x 7 font drawn for this package: space, digits, capitals, small letters and a little punctuation.  One glyph per entry, rows top to bottom.
_GLYPHS = {
    ' ': '...../...../...../...../...../...../.....',
    '0': '.###./#...#/#..##/#.#.#/##..#/#...#/.###.',
    '1': '..#../.##../..#../..#../..#../..#../.###.',
    '2': '.###./#...#/....#/...#./..#../.#.../#####',
    '3': '.###./#...#/....#/..##./....#/#...#/.###.',
    '4': '...#./..##./.#.#./#..#./#####/...#./...#.',
    '5': '#####/#..../####./....#/....#/#...#/.###.',
    '6': '..##./.#.../#..../####./#...#/#...#/.###.',
    '7': '#####/....#/...#./..#../..#../.#.../.#...',
    '8': '.###./#...#/#...#/.###./#...#/#...#/.###.',
    '9': '.###./#...#/#...#/.####/....#/...#./.##..',
    ':': '...../..#../..#../...../..#../..#../.....',
    '.': '...../...../...../...../...../.##../.##..',
    '-': '...../...../...../.###./...../...../.....',
    '%': '##..#/##.#./...#./..#../.#.../.#.##/#..##',
    '/': '....#/....#/...#./..#../.#.../#..../#....',
    'A': '..#../.#.#./#...#/#...#/#####/#...#/#...#',
    'B': '####./#...#/#...#/####./#...#/#...#/####.',
    'C': '.###./#...#/#..../#..../#..../#...#/.###.',
    'D': '###../#..#./#...#/#...#/#...#/#..#./###..',
    'E': '#####/#..../#..../###../#..../#..../#####',
    'F': '#####/#..../#..../###../#..../#..../#....',
    'G': '.###./#...#/#..../#.###/#...#/#...#/.###.',
    'H': '#...#/#...#/#...#/#####/#...#/#...#/#...#',
    'I': '.###./..#../..#../..#../..#../..#../.###.',
    'J': '..###/...#./...#./...#./...#./#..#./.##..',
    'K': '#...#/#..#./#.#../##.../#.#../#..#./#...#',
    'L': '#..../#..../#..../#..../#..../#..../#####',
    'M': '#...#/##.##/#.#.#/#.#.#/#...#/#...#/#...#',
    'N': '#...#/##..#/#.#.#/#..##/#...#/#...#/#...#',
    'O': '.###./#...#/#...#/#...#/#...#/#...#/.###.',
    'P': '####./#...#/#...#/####./#..../#..../#....',
    'Q': '.###./#...#/#...#/#...#/#.#.#/#..#./.##.#',
    'R': '####./#...#/#...#/####./#.#../#..#./#...#',
    'S': '.####/#..../#..../.###./....#/....#/####.',
    'T': '#####/..#../..#../..#../..#../..#../..#..',
    'U': '#...#/#...#/#...#/#...#/#...#/#...#/.###.',
    'V': '#...#/#...#/#...#/#...#/#...#/.#.#./..#..',
    'W': '#...#/#...#/#...#/#.#.#/#.#.#/##.##/#...#',
    'X': '#...#/#...#/.#.#./..#../.#.#./#...#/#...#',
    'Y': '#...#/#...#/.#.#./..#../..#../..#../..#..',
    'Z': '#####/....#/...#./..#../.#.../#..../#####',
    'a': '...../...../.###./....#/.####/#...#/.####',
    'b': '#..../#..../#.##./##..#/#...#/#...#/####.',
    'c': '...../...../.###./#..../#..../#...#/.###.',
    'd': '....#/....#/.##.#/#..##/#...#/#...#/.####',
    'e': '...../...../.###./#...#/#####/#..../.###.',
    'f': '..##./.#..#/.#.../###../.#.../.#.../.#...',
    'g': '...../.####/#...#/#...#/.####/....#/.###.',
    'h': '#..../#..../#.##./##..#/#...#/#...#/#...#',
    'i': '..#../...../.##../..#../..#../..#../.###.',
    'j': '...#./...../..##./...#./...#./#..#./.##..',
    'k': '#..../#..../#..#./#.#../##.../#.#../#..#.',
    'l': '.##../..#../..#../..#../..#../..#../.###.',
    'm': '...../...../##.#./#.#.#/#.#.#/#...#/#...#',
    'n': '...../...../#.##./##..#/#...#/#...#/#...#',
    'o': '...../...../.###./#...#/#...#/#...#/.###.',
    'p': '...../####./#...#/#...#/####./#..../#....',
    'q': '...../.####/#...#/#...#/.####/....#/....#',
    'r': '...../...../#.##./##..#/#..../#..../#....',
    's': '...../...../.####/#..../.###./....#/####.',
    't': '.#.../.#.../###../.#.../.#.../.#..#/..##.',
    'u': '...../...../#...#/#...#/#...#/#..##/.##.#',
    'v': '...../...../#...#/#...#/#...#/.#.#./..#..',
    'w': '...../...../#...#/#...#/#.#.#/#.#.#/.#.#.',
    'x': '...../...../#...#/.#.#./..#../.#.#./#...#',
    'y': '...../#...#/#...#/#...#/.####/....#/.###.',
    'z': '...../...../#####/...#./..#../.#.../#####',
}
FONT_FIRST, FONT_COUNT = 32, 95


def font_table():
    """[95, 7] uint8 for the characters 32 .. 126: bit 4 of a row = its leftmost pixel; a character without a drawing is blank."""
    out = np.zeros((FONT_COUNT, 7), dtype=np.uint8)
    for ch, art in _GLYPHS.items():
        rows = art.split('/')
        assert len(rows) == 7 and all(len(r) == 5 and set(r) <= set('#.') for r in rows), ch
        out[ord(ch) - FONT_FIRST] = [int(r.replace('#', '1').replace('.', '0'), 2) for r in rows]
    return out


def text_geometry(H):
    """(glyph pixel size, x of the first cell, y of the five lines): the 40-pixel font and the lines at (10, 10 + 50 k) of the 1000-pixel window, scaled by H / 1000."""
    return max(1, 40 * H // 8000), 10 * H // 1000, [(10 + 50 * k) * H // 1000 for k in range(TEXT_LINES)]


class Renderer:
    """The raw points of one room on the device, one visibility buffer, frames on demand."""

    def __init__(self, xyz, unequalized_idx, n, width=1000, height=1000, point_size=5, device=None):
        import torch
        from . import _lib
        self.torch, self._lib, self.lib = torch, _lib, _lib.load()
        if point_size < 1 or point_size % 2 == 0:
            raise ValueError('point size %d: a point is a square of odd side, centred on its pixel' % point_size)
        self.dev = torch.device(device if device is not None else 'cuda')
        self.W, self.H, self.size, self.n = int(width), int(height), int(point_size), int(n)
        xyz = np.ascontiguousarray(np.asarray(xyz, dtype=np.float32)[:, :3])
        uneq = np.ascontiguousarray(unequalized_idx, dtype=np.int32)
        if len(uneq) != len(xyz) or (len(uneq) and (uneq.min() < 0 or uneq.max() >= n)):
            raise ValueError('unequalized_idx must name one of the %d equalised points for each of the %d raw points' % (n, len(xyz)))
        self.M = len(xyz)
        self.d_xyz = torch.from_numpy(xyz).to(self.dev)
        self.d_uneq = torch.from_numpy(uneq).to(self.dev)
        self.d_vis = torch.empty(self.H * self.W, dtype=torch.int64, device=self.dev)
        self.d_luts = torch.from_numpy(luts()).to(self.dev)
        self.d_font = torch.from_numpy(font_table()).to(self.dev)
        self.palette = palette()
        self.has_vis = False

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    def build_visibility(self, eye=CAMERA, centre=LOOK_AT, up=UP):
        m = np.ascontiguousarray(camera_matrix(self.W, self.H, eye, centre, up).reshape(16))
        self._lib.check(self.lib.lrg_render_visibility(ctypes.c_void_p(self.d_xyz.data_ptr()), self.M, m.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                       self.W, self.H, self.size, ctypes.c_void_p(self.d_vis.data_ptr()), self._stream()),
                        'lrg_render_visibility')
        self.has_vis = True
        return self.d_vis

    def shade(self, index, frame_lut, texts=None):
        """index: device uint8 [T, stride >= n]; frame_lut: per frame LUT_STEP / LUT_SEG; texts: per frame None or five strings.
        -> device uint8 [T, H, W] of palette entries."""
        torch = self.torch
        if not self.has_vis:
            self.build_visibility()
        T = int(index.shape[0])
        assert index.dtype == torch.uint8 and index.dim() == 2 and index.is_contiguous() and index.shape[1] >= self.n and len(frame_lut) == T
        out = torch.empty((T, self.H, self.W), dtype=torch.uint8, device=self.dev)
        if T == 0:
            return out
        d_fl = torch.tensor([int(x) for x in frame_lut], dtype=torch.int32, device=self.dev)
        d_text = None
        if texts is not None and any(texts):
            assert len(texts) == T
            d_text = torch.from_numpy(text_block(texts)).to(self.dev)
        self._lib.check(self.lib.lrg_render_shade(
            ctypes.c_void_p(self.d_vis.data_ptr()), ctypes.c_void_p(self.d_uneq.data_ptr()), self.M, self.n, self.W, self.H, T,
            ctypes.c_void_p(index.data_ptr()), int(index.shape[1]), ctypes.c_void_p(self.d_luts.data_ptr()), 2, ctypes.c_void_p(d_fl.data_ptr()),
            ctypes.c_void_p(d_text.data_ptr()) if d_text is not None else None, TEXT_LEN, ctypes.c_void_p(self.d_font.data_ptr()), FONT_FIRST, FONT_COUNT,
            WHITE, ctypes.c_void_p(out.data_ptr()), self._stream()), 'lrg_render_shade')
        return out
