"""restatement of Mirostat v2's contract (include/gten_hip_mirostat.h), on tests/nucleus_ref.py and tests/sample_ref.py.

lg16, the update and the Q16 conversion are Python integers: the definition itself.  lg16_np is the same loop on numpy uint64 arrays, for
whole rows (tests/test_mirostat_cpu.py holds it to lg16).  a_j = (y_j - max y) / temp is numpy f32, the device's expression bit for bit;
q_j comes from float64 exp here and from f32 expf on the device, so a candidate's mass may differ by expf's error: `sure` says per
candidate whether that error can move it across the threshold, and a row is `near` when it can for some candidate."""
import math

import numpy as np

import nucleus_ref as nref

Q = 16
ONE = 1 << Q
MU_MAX = 64 << Q
MU_DEFAULT = -(1 << 31)
MASS_BITS = nref.MASS_BITS
INFO = np.dtype([("Z", np.uint64), ("Zk", np.uint64), ("q_id", np.uint64), ("n_cand", np.int32), ("n_keep", np.int32), ("s", np.int32),
                 ("mu_next", np.int32), ("pad", np.int32, (2,))])
OK, BAD_TAU, BAD_ETA = 0, 1, 2


def lg16(x):
    """the definition, for an integer x >= 1"""
    x = int(x)
    assert x >= 1
    e = x.bit_length() - 1
    m = x >> (e - 31) if e >= 31 else x << (31 - e)
    f = 0
    for _ in range(Q):
        m = (m * m) >> 31
        f <<= 1
        if m >= 1 << 32:
            f |= 1
            m >>= 1
    return (e << Q) | f


def lg16_np(x):
    """lg16 of every element of a uint64 array (all >= 1), as int64"""
    x = np.asarray(x, dtype=np.uint64)
    assert (x >= 1).all()
    t, e = x.copy(), np.zeros(x.shape, np.uint64)
    for s in (32, 16, 8, 4, 2, 1):
        big = (t >> np.uint64(s)) > 0
        t = np.where(big, t >> np.uint64(s), t)
        e += big.astype(np.uint64) * np.uint64(s)
    ei = e.astype(np.int64)
    m = (x >> np.maximum(ei - 31, 0).astype(np.uint64)) << np.maximum(31 - ei, 0).astype(np.uint64)
    f = np.zeros(x.shape, np.uint64)
    for _ in range(Q):
        m = (m * m) >> np.uint64(31)                                  # m < 2^32: the product fits 64 bits
        f <<= np.uint64(1)
        two = m >= np.uint64(1 << 32)
        f |= two.astype(np.uint64)
        m = np.where(two, m >> np.uint64(1), m)
    return ((e << np.uint64(Q)) | f).astype(np.int64)


def update(mu, s, tau_q, eta_q):
    """mu' = clamp(mu - ((eta_q * (s - tau_q)) >> 16), -MU_MAX, MU_MAX); Python's >> on a negative integer is the floor"""
    return max(-MU_MAX, min(MU_MAX, int(mu) - ((int(eta_q) * (int(s) - int(tau_q))) >> Q)))


def q16(tau, eta):
    """(code, tau_q, eta_q): 0 < tau <= 32, 0 < eta <= 1 as f32, both finite; lrint rounds halves to even, as np.rint does"""
    tau, eta = np.float32(tau), np.float32(eta)
    if not (tau > 0 and tau <= 32):
        return BAD_TAU, None, None
    if not (eta > 0 and eta <= 1):
        return BAD_ETA, None, None
    return OK, int(np.rint(np.float64(tau) * 65536.0)), int(np.rint(np.float64(eta) * 65536.0))


class Step:
    """everything the contract defines for one row (top_k >= 1) under the threshold mu"""

    def __init__(self, y, top_k, temp, mu, tau_q, eta_q):
        self.y, self.top_k, self.temp, self.mu, self.tau_q, self.eta_q = np.asarray(y, np.float32), int(top_k), float(temp), int(mu), int(tau_q), int(eta_q)
        self.c = nref.order(self.y, top_k)
        self.a = nref.scores(self.y, self.c, temp)
        self.q = nref.masses(self.a)
        self.n_cand = len(self.c)
        self.Z = int(self.q.sum(dtype=np.uint64))                                      # exact: at most 65535 terms of at most 2^36
        assert int(self.q[0]) == 1 << MASS_BITS
        self.L = lg16(self.Z) - self.mu
        has = self.q >= 1
        lg = np.full(self.n_cand, -1, np.int64)
        lg[has] = lg16_np(self.q[has])
        keep = has & (lg >= self.L)
        keep[0] = True
        self.n_keep = int(keep.sum())
        self.prefix = bool(keep[: self.n_keep].all())                                  # F is the first n_keep of C
        # what expf's error can move: d_j per mass, dl on the sum
        self.dl = math.ceil(nref.delta(self.Z, self.n_cand))
        d = (self.q >> np.uint64(22)) + np.uint64(2)
        l_hi = lg16(self.Z + self.dl + 1) - self.mu
        l_lo = lg16(max(1, self.Z - self.dl - 1)) - self.mu
        low = self.q > d                                                               # q - d >= 1
        lg_low = np.full(self.n_cand, -1, np.int64)
        lg_low[low] = lg16_np(self.q[low] - d[low])
        self.surely_kept = low & (lg_low >= l_hi)
        self.surely_dropped = lg16_np(self.q + d) < l_lo
        self.surely_kept[0], self.surely_dropped[0] = True, False
        self.near = bool((~self.surely_kept & ~self.surely_dropped).any())
        self.n_lo, self.n_hi = int(self.surely_kept.sum()), int((~self.surely_dropped).sum())

    def consistent(self, n_dev):
        """n_dev is a kept length some masses within expf's error of these would give"""
        return self.n_lo <= n_dev <= self.n_hi

    def outcome(self, id_, n_keep=None):
        """(Zk, q_id, s, mu') had `id_` been drawn from the first n_keep of C (default: the restatement's own n_keep)"""
        n_keep = self.n_keep if n_keep is None else n_keep
        Zk = int(self.q[:n_keep].sum(dtype=np.uint64))
        at = self.c[:n_keep].tolist().index(int(id_))
        q_id = int(self.q[at])
        s = lg16(Zk) - lg16(q_id)
        return Zk, q_id, s, update(self.mu, s, self.tau_q, self.eta_q)

    def draw(self, seed, stream, pos, n_keep=None):
        """(id, gap) of the draw over the first n_keep of C"""
        return nref.draw(self.y, self.top_k, self.temp, seed, stream, pos, self.n_keep if n_keep is None else n_keep)


def chain_rows(n_steps, n_vocab, seed=23):
    """the feedback chain's rows: N(0, 3^2) logits"""
    return (np.random.default_rng(seed).standard_normal((n_steps, n_vocab)) * 3.0).astype(np.float32)


def chain(rows, temp, tau_q, eta_q, feedback, seed=77, stream=5):
    """the surprises s of a chain over `rows` with top_k = n_vocab, row i at position i + 1, mu starting at 2 tau and -- with
    feedback -- following the update; returns (s per step, whether any step was near)"""
    mu, out, near = 2 * tau_q, [], False
    for i, y in enumerate(rows):
        st = Step(y, len(y), temp, mu, tau_q, eta_q)
        id_, _ = st.draw(seed, stream, i + 1)
        _, _, s, mu_next = st.outcome(id_)
        out.append(s)
        near |= st.near
        if feedback:
            mu = mu_next
    return out, near


def miss(s, tau_q):
    """|mean s - tau| over the second half of a chain, in bits"""
    half = s[len(s) // 2:]
    return abs(sum(half) / len(half) - tau_q) / ONE
