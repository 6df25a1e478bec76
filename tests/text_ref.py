"""NumPy / Python twin of the integer algorithm of csrc/lrg_text_fmt.h: '%f' of a float32 without one floating-point
operation.  It is the text the kernel is read against; tests/test_text_host.py holds it to Python's own '%f'.

    bits -> sign, m, e        subnormal: m = mantissa, e = -149; normal: m = mantissa | 2^23, e = exponent - 150
    N = m * 15625 ; s = e + 6
    s >= 0 : q = N << s       (|x| < 2^40, so q < 2^60)
    s <  0 : k = -s ; q = N >> k ; rem = low k bits of N ; half = 2^(k - 1) ; round half to even   (k >= 64: q = 0)
    text = ['-' if the sign bit is set] + decimal(q // 10^6) + '.' + six digits of q % 10^6
"""
import numpy as np

LRG_TEXT_MAX_LINE = 102
LIMIT_EXPONENT = 127 + 40          # |x| >= 2^40, inf and NaN: not encoded


def scaled(bits):
    """(sign bit, q) of one float32 bit pattern, or None where the device refuses the value."""
    bits = int(bits)
    sign, ex, man = bits >> 31, (bits >> 23) & 0xff, bits & 0x7fffff
    if ex >= LIMIT_EXPONENT:
        return None
    m, e = (man | 0x800000, ex - 150) if ex else (man, -149)
    N, s = m * 15625, e + 6
    if s >= 0:
        return sign, N << s
    k = -s
    if k >= 64:
        return sign, 0
    q, rem, half = N >> k, N & ((1 << k) - 1), 1 << (k - 1)
    if rem > half or (rem == half and (q & 1)):
        q += 1
    return sign, q


def format_f(value):
    """'%f' % value for a float32 value, from its bits; None if refused."""
    r = scaled(np.asarray(value, dtype=np.float32).view(np.uint32))
    if r is None:
        return None
    sign, q = r
    return ('-' if sign else '') + '%d.%06d' % (q // 1000000, q % 1000000)


def scaled_many(values):
    """q and sign of a float32 array, vectorised (uint64; the shifts as the kernel does them).  Refused values give q = 2^64 - 1."""
    bits = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32).astype(np.uint64)
    sign = (bits >> np.uint64(31)).astype(np.int64)
    ex = ((bits >> np.uint64(23)) & np.uint64(0xff)).astype(np.int64)
    man = bits & np.uint64(0x7fffff)
    m = np.where(ex > 0, man | np.uint64(0x800000), man)
    s = np.where(ex > 0, ex - 150, -149) + 6
    N = m * np.uint64(15625)
    left = N << np.clip(s, 0, 22).astype(np.uint64)
    k = np.clip(-s, 1, 63).astype(np.uint64)
    q = N >> k
    rem, half = N & ((np.uint64(1) << k) - np.uint64(1)), np.uint64(1) << (k - np.uint64(1))
    q = q + ((rem > half) | ((rem == half) & ((q & np.uint64(1)) == 1))).astype(np.uint64)
    q = np.where(-s >= 64, np.uint64(0), q)
    q = np.where(s >= 0, left, q)
    return sign, np.where(ex >= LIMIT_EXPONENT, np.uint64(2 ** 64 - 1), q)


def format_many(values):
    sign, q = scaled_many(values)
    return [None if int(v) == 2 ** 64 - 1 else ('-' if s else '') + '%d.%06d' % (int(v) // 1000000, int(v) % 1000000) for s, v in zip(sign, q)]


def line(xyz, rgb, fmt='ply'):
    """One vertex line, or None where the row is refused."""
    f = [format_f(v) for v in xyz]
    if any(t is None for t in f):
        return None
    r, g, b = (int(c) for c in rgb)
    if fmt == 'pcd':
        if not all(0 <= c <= 255 for c in (r, g, b)):
            return None
        return '%s %s %s %d\n' % (f[0], f[1], f[2], (r << 16) | (g << 8) | b)
    return '%s %s %s %d %d %d\n' % (f[0], f[1], f[2], r, g, b)
