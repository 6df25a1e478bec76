"""TensorFlow "bundle" (checkpoint V2) reader / writer -- the ``saver.restore(sess, MODEL_PATH)`` step of the reference
(test_region_grow.py:92-93, test_random_restart.py:106-107) without TensorFlow.

A checkpoint ``<prefix>`` is two files: ``<prefix>.index`` -- a LevelDB-format sorted string table whose keys are variable
names and whose values are serialized ``BundleEntryProto`` messages (dtype, shape, shard, offset, size, masked CRC-32C) --
and ``<prefix>.data-00000-of-00001`` -- the raw little-endian tensor bytes.  The reference's trained model is
``models/lrgnet_model5.ckpt`` (99 entries: the 32 ``lrg_*`` trainables, their Adam slots and three scalars; the data blob
is not distributed with the repository).  ``load_lrgnet_weights`` returns the ``name -> [1,Cin,Cout] / [Cout]`` dict that
``LrgNetHIP.load_weights`` takes; ``write_bundle`` writes a checkpoint the reference's ``tf.train.Saver`` can restore
(e.g. the synthetic weights used here, for cross-checking against the TensorFlow graph on a machine that has it).

Only what those files use is implemented: uncompressed table blocks, single-shard bundles, dense tensors.
"""
import os
import struct

import numpy as np

TABLE_MAGIC = 0xdb4775248b80fb57
_MASK_DELTA = 0xa282ead8
# tensorflow/core/framework/types.proto
DTYPES = {1: np.dtype('<f4'), 2: np.dtype('<f8'), 3: np.dtype('<i4'), 4: np.dtype('u1'), 5: np.dtype('<i2'),
          6: np.dtype('i1'), 9: np.dtype('<i8'), 10: np.dtype('?'), 17: np.dtype('<u2'), 22: np.dtype('<u4'),
          23: np.dtype('<u8')}
_DTYPE_ENUM = {v: k for k, v in DTYPES.items()}


class BundleError(ValueError):
    pass


# ---- CRC-32C (Castagnoli), slicing-by-8, and LevelDB's masking ----------------------------------------------------
def _make_tables():
    poly = 0x82f63b78
    t0 = np.zeros(256, dtype=np.uint32)
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ poly if c & 1 else c >> 1
        t0[i] = c
    tabs = [t0]
    for _ in range(7):
        prev = tabs[-1]
        tabs.append((prev >> np.uint32(8)) ^ t0[prev & np.uint32(0xff)])
    return [t.tolist() for t in tabs]


_T = _make_tables()


def crc32c(data, crc=0):
    b = memoryview(bytes(data) if not isinstance(data, (bytes, bytearray, memoryview)) else data).cast('B')
    c = crc ^ 0xffffffff
    n = len(b)
    i = 0
    t0, t1, t2, t3, t4, t5, t6, t7 = _T
    n8 = n - (n % 8)
    if n8:
        words = np.frombuffer(b[:n8], dtype='<u4').tolist()
        for j in range(0, len(words), 2):
            lo = words[j] ^ c
            hi = words[j + 1]
            c = (t7[lo & 0xff] ^ t6[(lo >> 8) & 0xff] ^ t5[(lo >> 16) & 0xff] ^ t4[lo >> 24] ^
                 t3[hi & 0xff] ^ t2[(hi >> 8) & 0xff] ^ t1[(hi >> 16) & 0xff] ^ t0[hi >> 24])
        i = n8
    while i < n:
        c = t0[(c ^ b[i]) & 0xff] ^ (c >> 8)
        i += 1
    return c ^ 0xffffffff


def mask_crc(crc):
    return ((((crc >> 15) | (crc << 17)) & 0xffffffff) + _MASK_DELTA) & 0xffffffff


def unmask_crc(masked):
    rot = (masked - _MASK_DELTA) & 0xffffffff
    return ((rot >> 17) | (rot << 15)) & 0xffffffff


# ---- varints / the two protobuf messages ---------------------------------------------------------------------------
def _get_varint(buf, pos):
    out = shift = 0
    while True:
        if pos >= len(buf):
            raise BundleError('truncated varint')
        b = buf[pos]
        pos += 1
        out |= (b & 0x7f) << shift
        if not b & 0x80:
            return out, pos
        shift += 7
        if shift > 70:
            raise BundleError('varint too long')


def _put_varint(v):
    out = bytearray()
    v &= (1 << 64) - 1
    while True:
        if v < 0x80:
            out.append(v)
            return bytes(out)
        out.append((v & 0x7f) | 0x80)
        v >>= 7


def _fields(buf):
    """Yield (field number, wire type, value) of one protobuf message (values: int or bytes)."""
    pos = 0
    while pos < len(buf):
        tag, pos = _get_varint(buf, pos)
        num, wt = tag >> 3, tag & 7
        if wt == 0:
            val, pos = _get_varint(buf, pos)
        elif wt == 1:
            val = struct.unpack_from('<Q', buf, pos)[0]
            pos += 8
        elif wt == 2:
            ln, pos = _get_varint(buf, pos)
            val = bytes(buf[pos:pos + ln])
            if len(val) != ln:
                raise BundleError('truncated field')
            pos += ln
        elif wt == 5:
            val = struct.unpack_from('<I', buf, pos)[0]
            pos += 4
        else:
            raise BundleError('unsupported wire type %d' % wt)
        yield num, wt, val


def _parse_shape(buf):
    dims = []
    for num, _, val in _fields(buf):
        if num == 2:                                  # repeated Dim dim = 2 { int64 size = 1; string name = 2 }
            size = 0
            for n2, _, v2 in _fields(val):
                if n2 == 1:
                    size = v2 - (1 << 64) if v2 >> 63 else v2
            dims.append(size)
        elif num == 3 and val:
            raise BundleError('unknown-rank shape')
    return tuple(dims)


class BundleEntry:
    __slots__ = ('dtype', 'shape', 'shard_id', 'offset', 'size', 'crc32c', 'sliced')

    def __init__(self):
        self.dtype, self.shape, self.shard_id, self.offset, self.size, self.crc32c, self.sliced = 0, (), 0, 0, 0, 0, False

    def __repr__(self):
        return 'BundleEntry(dtype=%d, shape=%s, shard=%d, offset=%d, size=%d, crc=0x%08x)' % (
            self.dtype, self.shape, self.shard_id, self.offset, self.size, self.crc32c)


def _parse_entry(buf):
    e = BundleEntry()
    for num, _, val in _fields(buf):                  # tensorflow/core/protobuf/tensor_bundle.proto
        if num == 1:
            e.dtype = val
        elif num == 2:
            e.shape = _parse_shape(val)
        elif num == 3:
            e.shard_id = val
        elif num == 4:
            e.offset = val
        elif num == 5:
            e.size = val
        elif num == 6:
            e.crc32c = val
        elif num == 7:
            e.sliced = True
    return e


def _encode_entry(dtype_enum, shape, offset, size, crc_masked):
    dims = b''.join(b'\x12' + _put_varint(len(d)) + d for d in (b'\x08' + _put_varint(int(s)) for s in shape))
    out = b'\x08' + _put_varint(dtype_enum) + b'\x12' + _put_varint(len(dims)) + dims
    if offset:
        out += b'\x20' + _put_varint(offset)
    out += b'\x28' + _put_varint(size) + b'\x35' + struct.pack('<I', crc_masked)
    return out


# ---- the sorted string table ---------------------------------------------------------------------------------------
def _read_block(data, offset, size, verify):
    raw = data[offset:offset + size]
    trailer = data[offset + size:offset + size + 5]
    if len(raw) != size or len(trailer) != 5:
        raise BundleError('table block out of range')
    if trailer[0] != 0:
        raise BundleError('compressed table blocks (type %d) are not supported' % trailer[0])
    if verify:
        want = struct.unpack('<I', trailer[1:5])[0]
        if mask_crc(crc32c(trailer[:1], crc32c(raw))) != want:
            raise BundleError('table block checksum mismatch at offset %d' % offset)
    return raw


def _block_entries(block):
    if len(block) < 4:
        raise BundleError('table block too small')
    nrestarts = struct.unpack_from('<I', block, len(block) - 4)[0]
    end = len(block) - 4 - 4 * nrestarts
    if end < 0:
        raise BundleError('bad restart array')
    pos, key = 0, b''
    while pos < end:
        shared, pos = _get_varint(block, pos)
        non_shared, pos = _get_varint(block, pos)
        vlen, pos = _get_varint(block, pos)
        if shared > len(key) or pos + non_shared + vlen > end:
            raise BundleError('corrupt table entry')
        key = key[:shared] + bytes(block[pos:pos + non_shared])
        pos += non_shared
        yield key, bytes(block[pos:pos + vlen])
        pos += vlen


def read_table(path, verify=True):
    """key (bytes) -> value (bytes) of a LevelDB-format table file, in key order."""
    data = open(path, 'rb').read()
    if len(data) < 48:
        raise BundleError('%s: too small for a table' % path)
    footer = data[-48:]
    if struct.unpack('<Q', footer[40:])[0] != TABLE_MAGIC:
        raise BundleError('%s: bad table magic' % path)
    pos = 0
    _, pos = _get_varint(footer, pos)                 # metaindex handle (unused)
    _, pos = _get_varint(footer, pos)
    ioff, pos = _get_varint(footer, pos)
    isize, pos = _get_varint(footer, pos)
    out = {}
    for _, handle in _block_entries(_read_block(data, ioff, isize, verify)):
        boff, p = _get_varint(handle, 0)
        bsize, p = _get_varint(handle, p)
        for k, v in _block_entries(_read_block(data, boff, bsize, verify)):
            out[k] = v
    return out


def _build_block(items, restart_interval=16):
    out = bytearray()
    restarts = []
    prev = b''
    for i, (k, v) in enumerate(items):
        shared = 0
        if i % restart_interval == 0:
            restarts.append(len(out))
        else:
            while shared < min(len(prev), len(k)) and prev[shared] == k[shared]:
                shared += 1
        out += _put_varint(shared) + _put_varint(len(k) - shared) + _put_varint(len(v)) + k[shared:] + v
        prev = k
    if not restarts:
        restarts = [0]
    for r in restarts:
        out += struct.pack('<I', r)
    out += struct.pack('<I', len(restarts))
    return bytes(out)


def write_table(path, items):
    """items: iterable of (key bytes, value bytes) in strictly increasing key order; one data block."""
    items = list(items)
    for a, b in zip(items, items[1:]):
        if not a[0] < b[0]:
            raise BundleError('table keys must be strictly increasing')
    out = bytearray()

    def emit(block):
        off = len(out)
        out.extend(block)
        out.extend(b'\x00' + struct.pack('<I', mask_crc(crc32c(b'\x00', crc32c(block)))))
        return _put_varint(off) + _put_varint(len(block))

    data_handle = emit(_build_block(items))
    meta_handle = emit(_build_block([]))
    last_key = items[-1][0] if items else b''
    index_handle = emit(_build_block([(last_key, data_handle)], restart_interval=1))
    footer = meta_handle + index_handle
    footer += b'\x00' * (40 - len(footer)) + struct.pack('<Q', TABLE_MAGIC)
    out.extend(footer)
    with open(path, 'wb') as f:
        f.write(bytes(out))


# ---- bundles -------------------------------------------------------------------------------------------------------
def _data_path(prefix, shard, num_shards):
    return '%s.data-%05d-of-%05d' % (prefix, shard, num_shards)


def read_bundle_index(prefix, verify=True):
    """-> (header dict, {variable name: BundleEntry}) of ``<prefix>.index``."""
    table = read_table(prefix + '.index', verify=verify)
    if b'' not in table:
        raise BundleError('%s.index: no bundle header' % prefix)
    header = dict(num_shards=1, endianness=0)
    for num, _, val in _fields(table[b'']):
        if num == 1:
            header['num_shards'] = val
        elif num == 2:
            header['endianness'] = val
    if header['endianness'] != 0:
        raise BundleError('big-endian bundles are not supported')
    entries = {k.decode('utf-8'): _parse_entry(v) for k, v in table.items() if k != b''}
    return header, entries


def load_bundle(prefix, names=None, verify=True):
    """name -> ndarray for the named variables (default: all dense ones) of checkpoint ``prefix``."""
    header, entries = read_bundle_index(prefix, verify=verify)
    if names is None:
        names = [n for n, e in entries.items() if not e.sliced and e.dtype in DTYPES]
    out = {}
    files = {}
    try:
        for name in names:
            if name not in entries:
                raise KeyError('%s: no variable named %r' % (prefix, name))
            e = entries[name]
            if e.sliced:
                raise BundleError('%s: partitioned variables are not supported' % name)
            if e.dtype not in DTYPES:
                raise BundleError('%s: unsupported dtype enum %d' % (name, e.dtype))
            dt = DTYPES[e.dtype]
            count = int(np.prod(e.shape, dtype=np.int64)) if e.shape else 1
            if count * dt.itemsize != e.size:
                raise BundleError('%s: %d bytes on disk for shape %s of %s' % (name, e.size, e.shape, dt))
            if e.shard_id not in files:
                files[e.shard_id] = open(_data_path(prefix, e.shard_id, header['num_shards']), 'rb')
            f = files[e.shard_id]
            f.seek(e.offset)
            raw = f.read(e.size)
            if len(raw) != e.size:
                raise BundleError('%s: data file truncated' % name)
            if verify and mask_crc(crc32c(raw)) != e.crc32c:
                raise BundleError('%s: CRC-32C mismatch (corrupt checkpoint data)' % name)
            out[name] = np.frombuffer(raw, dtype=dt).reshape(e.shape).copy()
    finally:
        for f in files.values():
            f.close()
    return out


def write_bundle(prefix, tensors):
    """Write ``{name: array}`` as a single-shard checkpoint ``<prefix>.index`` + ``<prefix>.data-00000-of-00001``."""
    names = sorted(tensors, key=lambda n: n.encode('utf-8'))
    header = b'\x08\x01' + b'\x1a\x02\x08\x01'        # num_shards = 1, (little endian,) version { producer: 1 }
    items = [(b'', header)]
    offset = 0
    d = os.path.dirname(prefix)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(_data_path(prefix, 0, 1), 'wb') as f:
        for name in names:
            a = np.asarray(tensors[name])
            a = np.ascontiguousarray(a).reshape(a.shape)          # (ascontiguousarray alone promotes scalars to [1])
            dt = a.dtype.newbyteorder('<') if a.dtype.itemsize > 1 else a.dtype
            if dt not in _DTYPE_ENUM:
                raise BundleError('%s: dtype %s cannot be stored' % (name, a.dtype))
            a = a.astype(dt, copy=False)
            raw = a.tobytes()
            enum = _DTYPE_ENUM[dt]
            items.append((name.encode('utf-8'), _encode_entry(enum, a.shape, offset, len(raw), mask_crc(crc32c(raw)))))
            f.write(raw)
            offset += len(raw)
    write_table(prefix + '.index', items)


def lrgnet_variable_shapes(feature_size=13, lite=0):
    """name -> TF shape of the 32 (lite: fewer) trainable variables (learn_region_grow_util.py:77-85,:107-159)."""
    from .lrgnet import CONV_CHANNELS, CONV2_CHANNELS
    lite = 0 if lite is None else int(lite)
    cc, c2 = CONV_CHANNELS[lite], CONV2_CHANNELS[lite]
    shapes = {}
    for pre in ('lrg_', 'lrg_neighbor_'):
        for i, c in enumerate(cc):
            shapes['%skernel%d' % (pre, i)] = (1, feature_size if i == 0 else cc[i - 1], c)
            shapes['%sbias%d' % (pre, i)] = (c,)
    for pre in ('lrg_add_', 'lrg_remove_'):
        for i, c in enumerate(c2):
            shapes['%skernel%d' % (pre, i)] = (1, cc[-1] * 2 + cc[1] if i == 0 else c2[i - 1], c)
            shapes['%sbias%d' % (pre, i)] = (c,)
        shapes['%skernel%d' % (pre, len(c2))] = (1, c2[-1], 2)
        shapes['%sbias%d' % (pre, len(c2))] = (2,)
    return shapes


def _saver_tensors(network, shapes, weights, adam_m, adam_v, step, beta1, beta2, no_slots=()):
    """The layout ``tf.compat.v1.train.Saver().save`` writes for a graph trained by AdamOptimizer: every variable of `shapes` (name ->
    TF shape; `network` names the graph in the errors), for all but `no_slots` its Adam slots ``<name>/Adam`` (first moment) and
    ``<name>/Adam_1`` (second moment; missing slots: zeros, a freshly built optimizer), ``beta1_power`` / ``beta2_power`` and
    ``Variable`` (the global step, int32)."""
    out = {}
    for k, shp in shapes.items():
        if k not in weights:
            raise KeyError('%s weight %s missing' % (network, k))
        w = np.asarray(weights[k], dtype=np.float32)
        if w.shape != tuple(shp):
            raise BundleError('%s has shape %s, %s needs %s' % (k, w.shape, network, shp))
        out[k] = w
        if k in no_slots:
            continue
        out[k + '/Adam'] = np.asarray(adam_m[k], dtype=np.float32).reshape(w.shape) if adam_m is not None else np.zeros_like(w)
        out[k + '/Adam_1'] = np.asarray(adam_v[k], dtype=np.float32).reshape(w.shape) if adam_v is not None else np.zeros_like(w)
    # TF1's AdamOptimizer creates the two accumulators AT beta (not 1) and multiplies them once per applied step, so a
    # checkpoint at global step t holds beta ** (t + 1); a freshly built optimizer (t = 0) holds beta itself -- with 1.0 there a
    # resumed reference run would compute lr * sqrt(1 - 1) / (1 - 1).
    out['beta1_power'] = np.float32(float(beta1) ** (int(step) + 1))
    out['beta2_power'] = np.float32(float(beta2) ** (int(step) + 1))
    out['Variable'] = np.int32(step)
    return out


def lrgnet_checkpoint_tensors(weights, adam_m=None, adam_v=None, step=0, beta1=0.9, beta2=0.999):
    """Everything ``tf.compat.v1.train.Saver().save`` writes for an LrgNet graph -- which is what ``Saver().restore``
    (test_region_grow.py:92-93) then asks for: the trainable variables, their Adam slots ``<name>/Adam`` (first moment) and
    ``<name>/Adam_1`` (second moment), ``beta1_power`` / ``beta2_power`` (learn_region_grow_util.py:188: AdamOptimizer) and
    ``Variable`` (the global step ``batch``, :187, int32) -- 99 entries for lite 0, the key set of models/lrgnet_model5.ckpt.index.
    weights / adam_m / adam_v: name -> array in the TF shapes (missing slots: zeros, a freshly built optimizer).  Whatever `weights`
    holds is written in the shapes it has: nothing is checked against an architecture.  The beta powers are beta ** (step + 1)
    (_saver_tensors says why)."""
    return _saver_tensors('LrgNet', {k: np.shape(w) for k, w in weights.items()}, weights, adam_m, adam_v, step, beta1, beta2)


def load_lrgnet_weights(prefix, feature_size=13, lite=0, verify=True):
    """The trainable variables of an LrgNet checkpoint (optimizer slots ignored), shapes checked against the
    architecture ``LrgNet(..., feature_size, lite)`` builds -- what ``saver.restore`` would have assigned."""
    shapes = lrgnet_variable_shapes(feature_size, lite)
    _, entries = read_bundle_index(prefix, verify=verify)
    for name, shp in shapes.items():
        if name not in entries:
            raise KeyError('%s: variable %s missing (wrong --lite / architecture?)' % (prefix, name))
        if tuple(entries[name].shape) != tuple(shp):
            raise BundleError('%s: checkpoint has shape %s, the network needs %s' % (name, entries[name].shape, shp))
        if entries[name].dtype != 1:
            raise BundleError('%s: not float32' % name)
    return load_bundle(prefix, names=list(shapes), verify=verify)


MCPNET_SHAPES = {'mcp_kernel1': (1, 6, 200), 'mcp_bias1': (200,), 'mcp_kernel2': (1, 200, 200), 'mcp_bias2': (200,),
                 'mcp_kernel3': (204, 200), 'mcp_bias3': (200,), 'mcp_kernel4': (200, 10), 'mcp_bias4': (10,)}
"""name -> TF shape of MCPNet's eight trainables (learn_region_grow_util.py:197-204; feature 6, hidden 200, embedding 10)."""


def load_mcpnet_weights(prefix, verify=True):
    """The eight ``mcp_*`` trainables of an MCPNet checkpoint (Adam slots and step ignored), shapes and dtypes checked, every
    tensor's bytes against its CRC-32C -- what ``saver.restore`` assigns at test_mcpnet.py:52."""
    _, entries = read_bundle_index(prefix, verify=verify)
    for name, shp in MCPNET_SHAPES.items():
        if name not in entries:
            raise KeyError('%s: variable %s missing (not an MCPNet checkpoint?)' % (prefix, name))
        if tuple(entries[name].shape) != tuple(shp):
            raise BundleError('%s: checkpoint has shape %s, MCPNet needs %s' % (name, entries[name].shape, shp))
        if entries[name].dtype != 1:
            raise BundleError('%s: not float32' % name)
    return load_bundle(prefix, names=list(MCPNET_SHAPES), verify=verify)


def mcpnet_checkpoint_tensors(weights, adam_m=None, adam_v=None, step=0, beta1=0.9, beta2=0.999):
    """Everything ``tf.compat.v1.train.Saver().save`` (train_mcpnet.py:227) writes for the MCPNet graph: the eight trainables, their
    Adam slots, the beta powers and ``Variable`` -- the 27 entries of the shipped models/mcpnet_model5.ckpt.index."""
    return _saver_tensors('MCPNet', MCPNET_SHAPES, weights, adam_m, adam_v, step, beta1, beta2)


POINTNET2_SA_MLPS = ((32, 32, 64), (64, 64, 128), (128, 128, 256), (256, 256, 512))     # train_pointnet.py:181-184
POINTNET2_FP_MLPS = ((256, 256), (256, 256), (256, 128), (128, 128, 128))               # :187-190


def pointnet2_variable_shapes(num_class=13, rgb_features=False):
    """name -> TF shape of PointNet2's 46 trainables (train_pointnet.py:133-134, :161-162, :194-200).  rgb_features: l0_points is
    the colour (:178; 6 and 131 input channels at layer1 and fa_layer4) instead of None (:177, the shipped models: 3 and 128)."""
    c0 = 3 if rgb_features else 0
    shapes = {}
    feat = [c0] + [m[-1] for m in POINTNET2_SA_MLPS]                  # l0 .. l4 feature widths
    for lv, mlp in enumerate(POINTNET2_SA_MLPS):
        cin = 3 + feat[lv]
        for i, c in enumerate(mlp):
            shapes['layer%d/kernel%d' % (lv + 1, i)] = (1, 1, cin, c)
            shapes['layer%d/bias%d' % (lv + 1, i)] = (c,)
            cin = c
    up = feat[4]                                                      # the interpolated width, then the skip's
    for lv, mlp in enumerate(POINTNET2_FP_MLPS):
        cin = up + feat[3 - lv]
        for i, c in enumerate(mlp):
            shapes['fa_layer%d/kernel%d' % (lv + 1, i)] = (1, 1, cin, c)
            shapes['fa_layer%d/bias%d' % (lv + 1, i)] = (c,)
            cin = c
        up = mlp[-1]
    shapes['kernel1'] = (1, 128, 128)
    shapes['bias1'] = (128,)
    shapes['kernel2'] = (1, 128, int(num_class))
    shapes['bias2'] = (int(num_class),)
    return shapes


def pointnet2_variant(shape_of):
    """(num_class, rgb_features) from a name -> shape mapping: the variant is read from the input channels of layer1/kernel0 (3 or
    6) and fa_layer4/kernel0 (128 or 131), which must agree; the class count is the last dimension of kernel2."""
    for name in ('layer1/kernel0', 'fa_layer4/kernel0', 'kernel2'):
        if name not in shape_of:
            raise BundleError('variable %s missing (not a PointNet2 checkpoint?)' % name)
    k0, k4, k2 = (tuple(shape_of[n]) for n in ('layer1/kernel0', 'fa_layer4/kernel0', 'kernel2'))
    if len(k0) != 4 or k0[2] not in (3, 6):
        raise BundleError('layer1/kernel0: shape %s has neither 3 (xyz) nor 6 (xyz and colour) input channels' % (k0,))
    if len(k4) != 4 or k4[2] not in (128, 131):
        raise BundleError('fa_layer4/kernel0: shape %s has neither 128 nor 131 input channels' % (k4,))
    if (k0[2] == 6) != (k4[2] == 131):
        raise BundleError('layer1/kernel0 %s and fa_layer4/kernel0 %s disagree about the colour features' % (k0, k4))
    if len(k2) != 3 or k2[2] < 1:
        raise BundleError('kernel2: shape %s is not (1, 128, num_class)' % (k2,))
    return int(k2[2]), k0[2] == 6


def load_pointnet2_weights(prefix, verify=True):
    """The 46 trainables of a PointNet2 checkpoint (``Variable`` and the Adam slots ignored) -- what ``saver.restore`` assigns at
    benchmarks.py:172.  The variant and the class count come from the checkpoint itself (pointnet2_variant); every shape and dtype
    is checked, every tensor's bytes against its CRC-32C.  A missing or mis-shaped variable raises BundleError naming it."""
    _, entries = read_bundle_index(prefix, verify=verify)
    try:
        num_class, rgb = pointnet2_variant({n: e.shape for n, e in entries.items()})
    except BundleError as e:
        raise BundleError('%s: %s' % (prefix, e))
    shapes = pointnet2_variable_shapes(num_class, rgb)
    for name, shp in shapes.items():
        if name not in entries:
            raise BundleError('%s: variable %s missing (not a PointNet2 checkpoint?)' % (prefix, name))
        if tuple(entries[name].shape) != tuple(shp):
            raise BundleError('%s: checkpoint has shape %s, PointNet2 needs %s' % (name, tuple(entries[name].shape), shp))
        if entries[name].dtype != 1:
            raise BundleError('%s: not float32' % name)
    return load_bundle(prefix, names=list(shapes), verify=verify)


def pointnet2_checkpoint_tensors(weights, adam_m=None, adam_v=None, step=0, beta1=0.9, beta2=0.999):
    """Everything ``tf.compat.v1.train.Saver().save`` (train_pointnet.py:367, :438) writes for the PointNet2 graph: the 46 trainables
    with their Adam slots ``<name>/Adam`` and ``<name>/Adam_1``, ``beta1_power`` / ``beta2_power`` and ``Variable`` (the global step
    ``batch``, :209) -- 141 entries, the key set of the shipped models/pointnet2_model5.ckpt.index for the xyz-only variant.  weights:
    name -> array in the TF shapes of pointnet2_variable_shapes (the variant and the class count are read from them); adam_m / adam_v:
    the slots (missing: zeros, a freshly built optimizer).  The beta powers follow pointnet_checkpoint_tensors: beta ** (step + 1)."""
    shapes = pointnet2_variable_shapes(*pointnet2_variant({k: np.shape(v) for k, v in weights.items()}))
    return _saver_tensors('PointNet2', shapes, weights, adam_m, adam_v, step, beta1, beta2)


POINTNET_NUM_POINT = 1024                                           # the row positions of a cell: the batch-norm tables' first axis
_POINTNET_MEAN = 'moments/Squeeze/ExponentialMovingAverage'
_POINTNET_VARIANCE = 'moments/Squeeze_1/ExponentialMovingAverage'


def pointnet_bn_names(j):
    """(beta, gamma, moving mean, moving variance) of the batch norm after hidden fc layer j (train_pointnet.py:63-84, :92).

    Block 0's names are those of the shipped models/pointnet_model5.ckpt.index.  A second block exists only in the network that
    train_pointnet.py builds today (NUM_FC_CHANNELS = [512, 256]), of which no checkpoint ships, so its names are INFERRED from
    TF 1's scoping rules and not pinned by a reference-made file: the re-entered ``variable_scope('bn')`` keeps the variable scope
    'bn' but opens the name scope 'bn_1', which names the ``tf.Variable``s ('bn_1/beta', 'bn_1/gamma') and the moments ops
    ('bn_1/moments/Squeeze'), and the moving averages take the variable scope in front of the op's name.  The loader therefore
    accepts for j >= 1 ANY entry that ends in the moments suffix and contains 'bn_<j>/' (load_pointnet_weights)."""
    scope = 'bn' if j == 0 else 'bn_%d' % j
    return ('%s/beta' % scope, '%s/gamma' % scope, 'bn/%s/%s' % (scope, _POINTNET_MEAN), 'bn/%s/%s' % (scope, _POINTNET_VARIANCE))


def pointnet_variable_shapes(conv_widths=(64, 64, 128, 512), fc_widths=(512,), num_class=13):
    """name -> TF shape of PointNet's trainables and batch-norm moving averages (train_pointnet.py:50-51, :66-71, :88-89, :96-97):
    conv_widths the 1x1 convolutions (the first reads the six input channels as a [1, 6] window), fc_widths the HIDDEN fc layers,
    each followed by a batch norm over the batch axis whose moving averages are [1024, c] tables, then fc_weights<len(fc_widths)>
    onto num_class.  The defaults are the shipped checkpoint; today's source builds ((64, 64, 64, 128, 1024), (512, 256)).  The
    names of the second batch-norm block are inferred, not pinned by a reference-made file: pointnet_bn_names."""
    conv, fc = tuple(int(c) for c in conv_widths), tuple(int(c) for c in fc_widths)
    shapes = {}
    for i, c in enumerate(conv):
        shapes['kernel%d' % i] = (1, 6, 1, c) if i == 0 else (1, 1, conv[i - 1], c)
        shapes['bias%d' % i] = (c,)
    k = conv[-1] + conv[1]                                            # the pooled-row difference joined with conv[1] (:59-61)
    for j, c in enumerate(fc + (int(num_class),)):
        shapes['fc_weights%d' % j] = (1, k, c)
        shapes['fc_bias%d' % j] = (c,)
        if j < len(fc):
            beta, gamma, mean, variance = pointnet_bn_names(j)
            shapes[beta] = shapes[gamma] = (c,)
            shapes[mean] = shapes[variance] = (POINTNET_NUM_POINT, c)
        k = c
    return shapes


def pointnet_variant(shape_of):
    """(conv_widths, fc_widths, num_class) from a name -> shape mapping.  The shipped checkpoint is not the network that
    train_pointnet.py builds today, so the architecture is read from the shapes: kernel0 (1, 6, 1, c0), then kernel<i>
    (1, 1, c_{i-1}, c_i) for as long as they exist (2 .. 5 layers), fc_weights<j> (1, k, n) for as long as they exist (2 .. 3; the
    last one's n is the class count, the others are fc_widths).  fc_weights0's k must be conv[-1] + conv[1] (the skip is conv[1],
    :60).  Every conv and hidden fc width is a multiple of 32; conv widths are at most 1024, hidden fc widths at most 512 (the
    kernels' limits).  BundleError names the offending variable."""
    def count(fmt):
        n = 0
        while fmt % n in shape_of:
            n += 1
        return n
    nk, nf = count('kernel%d'), count('fc_weights%d')
    if nk < 2:
        raise BundleError('variable kernel%d missing (not a PointNet checkpoint?)' % nk)
    if nk > 5:
        raise BundleError('kernel5: more than 5 convolutions')
    if nf < 2:
        raise BundleError('variable fc_weights%d missing (not a PointNet checkpoint?)' % nf)
    if nf > 3:
        raise BundleError('fc_weights3: more than 3 fc layers')
    conv = []
    for i in range(nk):
        s = tuple(shape_of['kernel%d' % i])
        want = (1, 6, 1) if i == 0 else (1, 1, conv[-1])
        if len(s) != 4 or s[:3] != want:
            raise BundleError('kernel%d: shape %s is not %s' % (i, s, want + ('c',)))
        if s[3] < 32 or s[3] % 32 or s[3] > 1024:
            raise BundleError('kernel%d: width %d is not a multiple of 32 in [32, 1024]' % (i, s[3]))
        conv.append(int(s[3]))
    widths = []
    k = conv[-1] + conv[1]
    for j in range(nf):
        s = tuple(shape_of['fc_weights%d' % j])
        if len(s) != 3 or s[:2] != (1, k):
            raise BundleError('fc_weights%d: shape %s is not (1, %d, n)%s' % (j, s, k, ' with %d = conv[-1] + conv[1]' % k if j == 0 else ''))
        if j < nf - 1 and (s[2] < 32 or s[2] % 32 or s[2] > 512):
            raise BundleError('fc_weights%d: width %d is not a multiple of 32 in [32, 512]' % (j, s[2]))
        if j == nf - 1 and not 1 <= s[2] <= 1024:
            raise BundleError('fc_weights%d: %d classes (1 .. 1024)' % (j, s[2]))
        widths.append(int(s[2]))
        k = s[2]
    return tuple(conv), tuple(widths[:-1]), widths[-1]


def _pointnet_entry_name(name, shp, shape_of):
    """The checkpoint's name for this repository's `name`: itself, or for a moving average of batch-norm block j >= 1 the unique
    entry of its shape that ends in the moments suffix and contains 'bn_<j>/'."""
    if name in shape_of:
        return name
    for suffix in (_POINTNET_MEAN, _POINTNET_VARIANCE):
        if name.endswith('/' + suffix) and not name.startswith('bn/bn/'):
            scope = name[len('bn/'):-len(suffix)]                     # 'bn_<j>/'
            named = [n for n in shape_of if n.endswith('/' + suffix) and scope in n]
            hits = [n for n in named if tuple(shape_of[n]) == tuple(shp)]
            if len(hits) == 1:
                return hits[0]
            if named and not hits:
                raise BundleError('%s: checkpoint has shape %s, PointNet needs %s' % (named[0], tuple(shape_of[named[0]]), tuple(shp)))
            if hits:
                raise BundleError('%s: %d entries match (%s)' % (name, len(hits), ', '.join(sorted(hits))))
    raise BundleError('variable %s missing (not a PointNet checkpoint?)' % name)


def load_pointnet_weights(prefix, verify=True):
    """PointNet's trainables and batch-norm moving averages (``Variable``, ``beta*_power`` and the Adam slots ignored) under this
    repository's names (pointnet_variable_shapes) -- what ``saver.restore`` assigns at benchmarks.py:172.  The architecture comes
    from the checkpoint itself (pointnet_variant); every shape and dtype is checked, every tensor's bytes against its CRC-32C.  A
    missing or mis-shaped variable raises BundleError naming it."""
    _, entries = read_bundle_index(prefix, verify=verify)
    shape_of = {n: tuple(e.shape) for n, e in entries.items()}
    try:
        shapes = pointnet_variable_shapes(*pointnet_variant(shape_of))
        found = {name: _pointnet_entry_name(name, shp, shape_of) for name, shp in shapes.items()}
    except BundleError as e:
        raise BundleError('%s: %s' % (prefix, e))
    for name, shp in shapes.items():
        if shape_of[found[name]] != tuple(shp):
            raise BundleError('%s: %s: checkpoint has shape %s, PointNet needs %s' % (prefix, found[name], shape_of[found[name]], shp))
        if entries[found[name]].dtype != 1:
            raise BundleError('%s: %s: not float32' % (prefix, found[name]))
    loaded = load_bundle(prefix, names=sorted(set(found.values())), verify=verify)
    return {name: loaded[found[name]] for name in shapes}


def pointnet_checkpoint_tensors(weights, adam_m=None, adam_v=None, step=0, beta1=0.9, beta2=0.999):
    """Everything ``tf.compat.v1.train.Saver().save`` (train_pointnet.py:367, :438) writes for the PointNet graph: the trainables
    (kernel*, bias*, fc_weights*, fc_bias*, every block's beta and gamma) with their Adam slots ``<name>/Adam`` and
    ``<name>/Adam_1``, the batch norms' moving averages (pointnet_bn_names; shadows of tensors, not trainable, so without slots),
    ``beta1_power`` / ``beta2_power`` and ``Variable`` (the global step ``batch``, :108) -- the key set of the shipped
    models/pointnet_model5.ckpt.index for that architecture.  weights: name -> array in the TF shapes under the names of
    pointnet_variable_shapes; adam_m / adam_v: the trainables' slots (missing: zeros, a freshly built optimizer).  The beta powers
    follow lrgnet_checkpoint_tensors: beta ** (step + 1)."""
    shapes = pointnet_variable_shapes(*pointnet_variant({k: np.shape(v) for k, v in weights.items()}))
    averages = set()
    j = 0
    while pointnet_bn_names(j)[2] in shapes:
        averages.update(pointnet_bn_names(j)[2:])
        j += 1
    return _saver_tensors('PointNet', shapes, weights, adam_m, adam_v, step, beta1, beta2, no_slots=averages)
