"""numpy restatement of the penalties' contract (include/gten_hip_penalty.h), in np.float32 operations: every
multiply, divide, add and subtract below is one IEEE f32 operation, as on the device, so the rows agree with it bit for bit.  What
follows the row -- candidates, cut, draw -- is tests/sample_ref.py and tests/nucleus_ref.py on y.
"""
import numpy as np

import bias_ref as bref
import sample_ref as sref

R_MIN, R_MAX, ADD_MAX, HISTORY_MAX = 0.125, 8.0, 100.0, 65535     # GTEN_HIP_PENALTY_*


def penalty_ok(r, freq, pres, start=0, last_n=0):
    f = lambda v: float(np.float32(v))                               # noqa: E731
    return bool(np.isfinite(f(r)) and R_MIN <= f(r) <= R_MAX and np.isfinite(f(freq)) and abs(f(freq)) <= ADD_MAX and
                np.isfinite(f(pres)) and abs(f(pres)) <= ADD_MAX and start >= 0 and last_n >= 0)


def is_on(r, freq, pres):
    return not (np.float32(r) == 1.0 and np.float32(freq) == 0.0 and np.float32(pres) == 0.0)


def window(n, start, last_n):
    """(lo, n): the positions counted for the id that will sit at position n"""
    lo = max(start, n - last_n if last_n > 0 else 0)
    return min(max(lo, 0), n), n


def counts(ids, n_vocab):
    """c_i over a window's ids; ids outside [0, n_vocab) are not counted"""
    ids = np.asarray(ids, np.int64).reshape(-1)
    ids = ids[(ids >= 0) & (ids < n_vocab)]
    return np.bincount(ids, minlength=n_vocab).astype(np.int64)


def penalised(x, c, r, freq, pres):
    """p: x where c == 0, otherwise (x > 0 ? x / r : x * r) - ((float)c * freq + pres)"""
    x = np.asarray(x, np.float32)
    r, freq, pres = np.float32(r), np.float32(freq), np.float32(pres)
    with np.errstate(all="ignore"):
        u = np.where(x > 0, (x / r).astype(np.float32), (x * r).astype(np.float32)).astype(np.float32)
        t = (np.asarray(c).astype(np.float32) * freq).astype(np.float32)
        t = (t + pres).astype(np.float32)
        p = (u - t).astype(np.float32)
    return np.where(np.asarray(c) > 0, p, x).astype(np.float32)


def row(x, ids, r, freq, pres, b=None):
    """y: the row the draw is made from -- p (x itself for (1, 0, 0)), or p + b under a table"""
    x = np.asarray(x, np.float32)
    p = penalised(x, counts(ids, x.size), r, freq, pres) if is_on(r, freq, pres) else x
    return p if b is None else bref.biased(p, b)


def decoder_row(x, tokens, n, r, freq, pres, start, last_n, b=None):
    """y of the decoder's step for context length n of a sequence whose ids so far are tokens[0, n)"""
    lo, hi = window(n, start, last_n)
    return row(x, np.asarray(tokens)[lo:hi], r, freq, pres, b)


def greedy(y):
    return sref.draw(y, 0, 1.0, 0, 0, 0)[0]
