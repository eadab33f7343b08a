"""numpy restatement of the top-p / min-p cut's contract (include/gten_hip_nucleus.h), on tests/sample_ref.py.

The order, the counts and the masses are integers.  a_j = (y_j - max y) / temp is formed in numpy f32, which is the device's
expression bit for bit (one IEEE subtraction, one IEEE division).  q_j = floor(exp(a_j) * 2^36) comes from float64 exp here and
from f32 expf on the device, so the two may differ by expf's error: delta() is the bound on what that can move a sum, and `near`
says whether a row's cut lies within it.
"""
import numpy as np

import sample_ref as sref

MASS_BITS = 36
INFO = np.dtype([("Z", np.uint64), ("n_cand", np.int32), ("n_nucleus", np.int32), ("n_minp", np.int32), ("n_keep", np.int32)])


def key(x):
    """the order-preserving integer image of f32 values, -0 == +0 (smp_key)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    return np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def order(y, top_k):
    """C in its order: the min(top_k, n) largest keys, key descending, index ascending"""
    y = np.asarray(y, dtype=np.float32)
    k = min(int(top_k), y.size)
    o = np.lexsort((np.arange(y.size), -key(y).astype(np.int64)))
    return o[:k]


def scores(y, c, temp):
    """a_j = (y_j - max y) / temp in f32 for the indices c"""
    y = np.asarray(y, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return ((y[c] - y.max()) / np.float32(temp)).astype(np.float32)


def masses(a):
    """q_j = floor(exp(a_j) * 2^36) as python-exact uint64 (float64 exp; -inf gives 0)"""
    w = np.exp(np.asarray(a, dtype=np.float64))
    return np.floor(w * float(1 << MASS_BITS)).astype(np.uint64)


def t_of(min_p):
    """t = (float)log((double)min_p), -inf for 0"""
    with np.errstate(divide="ignore"):
        return np.float32(np.log(np.float64(np.float32(min_p))))


def p_of(Z, top_p):
    """P = (uint64) floor((double)Z * (double)top_p): one f64 multiply"""
    return int(np.floor(np.float64(int(Z)) * np.float64(np.float32(top_p))))


def delta(Z, n_cand):
    """what expf's error can move a sum of masses by: two f32 ulps per term (2^-22 of each, 2^-21 Z as a round bound) plus one
    count per floor and one for the restatement's own floor"""
    return float(int(Z)) * 2.0 ** -21 + 2.0 * n_cand


class Cut:
    """everything the contract defines for one row"""

    def __init__(self, y, top_k, temp, top_p, min_p):
        self.c = order(y, top_k)
        self.a = scores(y, self.c, temp)
        self.q = masses(self.a)
        self.S = np.cumsum(self.q, dtype=np.uint64)                     # exact: n_vocab <= 65535 terms of at most 2^36
        self.Z = int(self.S[-1])
        self.n_cand = len(self.c)
        self.P = p_of(self.Z, top_p)
        if np.float32(top_p) == np.float32(1.0):
            self.n_nucleus = self.n_cand
        else:
            self.n_nucleus = max(1, int(np.searchsorted(self.S, np.uint64(self.P), side="left")) + 1)     # the first n with S[n - 1] >= P
        self.t = t_of(min_p)
        self.n_minp = int((self.a >= self.t).sum())
        self.n_keep = min(self.n_nucleus, self.n_minp)
        self.delta = delta(self.Z, self.n_cand)
        # near: the cut lies within delta of a prefix sum -- the device's n_nucleus may then differ
        n = self.n_nucleus
        below = int(self.S[n - 2]) if n >= 2 else None
        gaps = [int(self.S[n - 1]) - self.P] + ([self.P - below] if below is not None else [])
        self.near = np.float32(top_p) != np.float32(1.0) and min(gaps) <= self.delta

    def consistent(self, n_dev):
        """n_dev is a nucleus length some masses within delta of these would give"""
        if not 1 <= n_dev <= self.n_cand:
            return False
        hi = int(self.S[n_dev - 1]) >= self.P - self.delta
        lo = n_dev == 1 or int(self.S[n_dev - 2]) < self.P + self.delta
        return hi and lo


def draw(y, top_k, temp, seed, stream, pos, n_keep):
    """(id, gap) of the draw over the first n_keep of C: argmax of a_j + g_j in float64, the lower index winning ties; gap to the
    best other member (inf when alone)"""
    y = np.asarray(y, dtype=np.float32)
    f = np.sort(order(y, top_k)[:n_keep])
    ym = y.astype(np.float64)
    s = (ym[f] - ym.max()) / float(np.float32(temp)) + sref.gumbel(f, pos, stream, seed)
    best = int(np.argmax(s))
    rest = np.delete(s, best)
    return int(f[best]), (float(s[best] - rest.max()) if rest.size else np.inf)
