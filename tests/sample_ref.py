"""numpy restatement of the device top-k sampler's contract (csrc/gten_decode_sample.h).

Philox4x32-10 in integers, the uniform in f32 arithmetic exactly as the kernel forms it, the Gumbel noise and the
scores in float64.  The device scores in f32, so the two may disagree where two candidates' scores are within
rounding of each other: `draw` returns the runner-up's gap so that callers can excuse those near ties.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
U_MAX = np.float32(1.0) - np.float32(2.0 ** -24)


def philox4x32(ctr, key, rounds=10):
    """Random123's philox4x32 on scalar or array words; returns the four output words (uint64 arrays)."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in ctr]
    k0, k1 = (np.asarray(v, dtype=np.uint64) & MASK for v in key)
    for r in range(rounds):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        if r + 1 < rounds:
            k0 = (k0 + np.uint64(W0)) & np.uint64(MASK)
            k1 = (k1 + np.uint64(W1)) & np.uint64(MASK)
    return c


def uniform(j, pos, stream, seed):
    """u_j = f32((w >> 8) + 0.5) * 2^-24, capped below 1 (w = word 0 of Philox at counter (j, pos, stream, 0))."""
    seed = int(seed)
    w = philox4x32((np.asarray(j), pos, stream, 0), (seed & MASK, seed >> 32))[0]
    u = ((w >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    return np.minimum(u, U_MAX)


def gumbel(j, pos, stream, seed):
    u = uniform(j, pos, stream, seed).astype(np.float64)
    return -np.log(-np.log(u))


def candidates(x, top_k):
    """indices of the min(top_k, n) largest values, ties at the threshold to the lower index"""
    x = np.asarray(x, dtype=np.float32)
    k = min(int(top_k), x.size)
    order = np.lexsort((np.arange(x.size), -x.astype(np.float64)))   # value descending, index ascending
    return np.sort(order[:k])


def scores(x, top_k, temp, seed, stream, pos):
    """(candidate indices, their scores (x_j - max x) / temp + g_j in float64)"""
    x = np.asarray(x, dtype=np.float32)
    c = candidates(x, top_k)
    xm = x.astype(np.float64)
    s = (xm[c] - xm.max()) / float(np.float32(temp)) + gumbel(c, pos, stream, seed)
    return c, s


def draw(x, top_k, temp, seed, stream, pos):
    """(id, gap): the contract's id for one row, and the score gap to the best other candidate (inf when alone).
    top_k == 0: the greedy argmax (first maximum), gap inf."""
    x = np.asarray(x, dtype=np.float32)
    if top_k == 0:
        return int(np.argmax(x)), np.inf
    c, s = scores(x, top_k, temp, seed, stream, pos)
    best = int(np.argmax(s))                     # first maximum: c is ascending, so the lower index wins ties
    rest = np.delete(s, best)
    return int(c[best]), (float(s[best] - rest.max()) if rest.size else np.inf)


def score_of(x, j, temp, seed, stream, pos):
    """the score of one index (any index, candidate or not)"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    return float((x[j] - x.max()) / float(np.float32(temp)) + gumbel(np.asarray([j]), pos, stream, seed)[0])
