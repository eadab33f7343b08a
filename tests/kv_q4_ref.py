"""NumPy restatement of R, "Q4 of a Q8 block" (csrc/gten_kvq4_math.h): float64 inside, rounded to float32 at the two
divisions the definition names.  Rows are uint8 [n][blocks * 34], a block = f16 delta + 32 int8."""
import numpy as np


def round_rows(rows):
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    n = rows.shape[0]
    blk = rows.reshape(n, -1, 34)
    d = blk[:, :, :2].copy().view(np.float16)[:, :, 0]
    q = blk[:, :, 2:].view(np.int8).astype(np.float64)
    df = d.astype(np.float64)
    finite = np.isfinite(df)
    dz = np.where(finite, df, 0.0)
    m = np.abs(q).max(axis=2)
    x = (m * np.abs(dz) / 7.0).astype(np.float32)                       # the product is exact; ONE rounding, of the quotient
    with np.errstate(over="ignore"):
        d4 = np.minimum(x.astype(np.float16).astype(np.float64), 65504.0)  # f32 -> f16 to nearest even, an overflow stays the largest half
    d4 = np.where(finite & (x >= np.float32(2.0 ** -14)), d4, 0.0)
    safe = np.where(d4 > 0, d4, 1.0)
    r = np.rint((q * dz[:, :, None] / safe[:, :, None]).astype(np.float32).astype(np.float64))   # half to even
    q4 = np.where(d4[:, :, None] > 0, np.clip(r, -7, 7), 0.0).astype(np.int8)
    out = np.empty_like(blk)
    out[:, :, :2] = d4.astype(np.float16)[:, :, None].view(np.uint8)
    out[:, :, 2:] = q4.view(np.uint8)
    return out.reshape(n, -1)


def edge_rows(n_rows, n_blocks, seed):
    """random Q8 rows with the blocks the definition has cases for: all zero, a single non-zero, |q| = 127 and -128, tiny, huge,
    negative and non-finite deltas"""
    r = np.random.default_rng(seed)
    q = r.integers(-127, 128, (n_rows, n_blocks, 32)).astype(np.int8)
    d = (r.random((n_rows, n_blocks)) * 0.05 + 1e-4).astype(np.float16)
    q[0, 0] = 0
    q[0, 1 % n_blocks] = 0
    q[0, 1 % n_blocks, 5] = -3
    q[1 % n_rows, 0, 7] = 127
    q[1 % n_rows, 1 % n_blocks, 9] = -128
    flat_d = d.reshape(-1)
    specials = np.array([0x0000, 0x0001, 0x0007, 0x03ff, 0x0400, 0x7bff, 0x7000, 0x8400, 0x7c00, 0x7e00, 0xfc00], np.uint16).view(np.float16)
    flat_d[2:2 + len(specials)] = specials[:max(0, len(flat_d) - 2)]
    q.reshape(-1, 32)[2 + len(specials):2 + len(specials) + 4] //= 16    # small quants: several elements tie at the maximum
    rows = np.empty((n_rows, n_blocks, 34), np.uint8)
    rows[:, :, :2] = d[:, :, None].view(np.uint8)
    rows[:, :, 2:] = q.view(np.uint8)
    return rows.reshape(n_rows, -1)
