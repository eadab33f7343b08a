"""numpy restatement of the bias tables' contract (include/gten_hip_bias.h), on top of tests/sample_ref.py.

A table is a dense f32 row b; where it holds, y = x + b is formed in float32 (one add, as the kernel does) and the draw is
sample_ref's on y.  An entry of -inf bans its id: y is -inf there, it sorts below every finite value and its score is -inf.
"""
import numpy as np

import sample_ref as ref

TABLES = 16                      # GTEN_HIP_BIAS_TABLES
B_MAX = 1e30                     # GTEN_HIP_BIAS_MAX


def table(n_vocab, pairs=(), fill=0.0, allow=None):
    """the dense f32 row of a table request; allow=[ids]: fill -inf, those ids at 0 (pairs on top of that)"""
    if allow is not None:
        fill = -np.inf
    b = np.full(n_vocab, fill, np.float32)
    if allow is not None:
        b[np.asarray(list(allow), dtype=np.int64)] = 0.0
    for j, v in pairs:
        b[int(j)] = np.float32(v)
    return b


def table_ok(n_vocab, pairs=(), fill=0.0):
    """the request's validity: ids in range and not repeated, values finite with |b| <= B_MAX or -inf, not every id banned"""
    def value_ok(v):
        v = float(np.float32(v))
        return v == -np.inf or (np.isfinite(v) and abs(v) <= float(np.float32(B_MAX)))
    ids = [int(j) for j, _ in pairs]
    if any(j < 0 or j >= n_vocab for j in ids) or len(set(ids)) != len(ids):
        return False
    if not value_ok(fill) or not all(value_ok(v) for _, v in pairs):
        return False
    return bool((table(n_vocab, pairs, fill) > -np.inf).any())


def holds(b, until, pos):
    return b is not None and (until == 0 or pos < until)


def biased(x, b):
    """y = x + b in float32"""
    with np.errstate(invalid="ignore"):
        return (np.asarray(x, np.float32) + np.asarray(b, np.float32)).astype(np.float32)


def draw(x, b, top_k, temp, seed, stream, pos, until=0):
    """(id, gap) of the contract: sample_ref.draw on y where the table holds at `pos`, on x otherwise"""
    if not holds(b, until, pos):
        return ref.draw(x, top_k, temp, seed, stream, pos)
    with np.errstate(invalid="ignore"):
        return ref.draw(biased(x, b), top_k, temp, seed, stream, pos)


def score_of(x, b, j, temp, seed, stream, pos):
    with np.errstate(invalid="ignore"):
        return ref.score_of(biased(x, b), j, temp, seed, stream, pos)


def allowed(b):
    """the ids a table leaves open"""
    return np.flatnonzero(np.asarray(b) > -np.inf)
