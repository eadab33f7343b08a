"""NumPy restatement of R8 / E8 / R of the FP8 (E4M3) K / V shadows, from the contract and in integers: a magnitude in
units of 2^-24 is rounded, half to even, to whole steps of 2^max(k - 3, 15) units (2^k its leading bit), then clamped to 448."""
import numpy as np

_MAX = 7 << 30                                                   # 448 in units of 2^-24


def _top_bit(v):
    k = np.zeros(v.shape, np.int64)
    for j in range(1, 44):
        k += (v >> j) > 0
    return k


def r8(h):
    h = np.asarray(h, np.uint16).astype(np.int64)
    sign, e, m = h >> 15, (h >> 10) & 31, h & 1023
    v = np.where(e > 0, (1024 + m) << np.maximum(e - 1, 0), m)
    nan = (e == 31) & (m != 0)
    q = np.maximum(_top_bit(v) - 3, 15)
    n, rem, half = v >> q, v & ((1 << q) - 1), 1 << (q - 1)
    n = n + ((rem > half) | ((rem == half) & ((n & 1) == 1)))
    w = np.minimum(n << q, _MAX)
    k = _top_bit(w)
    code = np.where(k < 18, w >> 15, ((k - 17) << 3) | ((w >> np.maximum(k - 3, 0)) & 7))
    return np.where(nan, 0, (sign << 7) | code).astype(np.uint8)


def e8(c):
    c = np.asarray(c, np.uint8).astype(np.int64)
    sign, E, m = c >> 7, (c >> 3) & 15, c & 7
    w = np.where(E > 0, (8 + m) << (E + 14), m << 15)
    k = _top_bit(w)
    bits = ((k - 9) << 10) | (((w << 10) >> k) & 1023)
    return ((sign << 15) | np.where(w > 0, bits, 0)).astype(np.uint16)


def round_rows(rows):
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    return e8(r8(rows.view(np.uint16))).view(np.uint8).reshape(rows.shape)
