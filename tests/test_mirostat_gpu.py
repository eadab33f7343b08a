"""-m gpu: Mirostat v2 on the device (include/gten_hip_mirostat.h): the row operator.

The operator is held to tests/miro_ref.py.  n_cand exactly; Z within delta = 2^-21 Z + 2 |C| (expf's error: the restatement's masses come
from float64 exp); n_keep consistent on every row and EQUAL where no candidate lies within expf's error of the threshold
(tests/test_mirostat_cpu.py asserts that this is at least 90 % of the rows); Zk within delta of the restatement's masses of the device's
own n_keep (the device's single masses are not observable: only their sums and the drawn id's come back); the id to the restatement's draw over the device's own n_keep (tests/test_sampler_gpu.py's near-tie excuse only); and, from the
device's own integers, s and mu_next EXACTLY: that holds the device's lg16 and update to the definition bit for bit.  The decoder is
held to the operator in tests/test_mirostat_decoder_gpu.py."""
import numpy as np
import pytest

import bias_ref as bref
import mirostat_cases as cases
import miro_ref as ref
import nucleus_ref as nref
import sample_ref as sref
from gpu_common import hip  # noqa: F401
from test_bias_gpu import NINF, upload

pytestmark = pytest.mark.gpu

NEAR = 1e-4                                         # tests/test_sampler_gpu.py's near tie of two scores
LIMIT = 1024                                        # up to this many candidates smp_row_miro works on the candidates compacted into LDS,
                                                    # above it on the row: every edge is run on both sides
TAU, ETA, TAU_Q, ETA_Q = cases.TAU, cases.ETA, cases.TAU_Q, cases.ETA_Q


def check_row(y, k, temp, mu, seed, stream, pos, got_id, info, what, tau_q=TAU_Q, eta_q=ETA_Q):
    """one row of the operator against the restatement; returns (the row is near, the id needed the near-tie excuse)"""
    st = ref.Step(y, k, temp, mu, tau_q, eta_q)
    Z, Zk, q_id = int(info["Z"]), int(info["Zk"]), int(info["q_id"])
    n_cand, n_keep, s, mu_next = int(info["n_cand"]), int(info["n_keep"]), int(info["s"]), int(info["mu_next"])
    print(f"{what}: Z dev {Z} ref {st.Z} (diff {Z - st.Z}, delta {st.dl}) n_cand {n_cand} n_keep dev {n_keep} ref {st.n_keep} "
          f"[{st.n_lo}, {st.n_hi}] near {st.near} s {s} mu {mu} -> {mu_next}")
    assert n_cand == st.n_cand, what
    assert abs(Z - st.Z) <= st.dl, (what, Z, st.Z, st.dl)
    assert 1 <= n_keep <= n_cand and st.consistent(n_keep), (what, n_keep, st.n_lo, st.n_hi)
    if not st.near:
        assert n_keep == st.n_keep, (what, n_keep, st.n_keep)
    assert abs(Zk - int(st.q[:n_keep].sum(dtype=np.uint64))) <= st.dl, (what, Zk)
    want, _ = st.draw(seed, stream, pos, n_keep)
    excused = False
    kept = st.c[:n_keep].tolist()
    if got_id != want:
        assert got_id in kept, (what, got_id)
        gap = sref.score_of(y, want, temp, seed, stream, pos) - sref.score_of(y, got_id, temp, seed, stream, pos)
        assert 0.0 <= gap <= NEAR, (what, got_id, want, gap)
        excused = True
    q_ref = int(st.q[kept.index(got_id)])
    assert q_id >= 1 and abs(q_id - q_ref) <= (q_ref >> 22) + 2, (what, q_id, q_ref)
    # exactly, from the device's own integers
    assert s == ref.lg16(Zk) - ref.lg16(q_id), (what, s, Zk, q_id)
    assert mu_next == ref.update(mu, s, tau_q, eta_q), (what, mu_next, mu, s)
    assert not info["pad"].any()
    return bool(st.near), excused


# ------------------------------------------------------------------------------------------------------------ 1. the operator

@pytest.mark.parametrize("n_vocab", cases.VOCABS)
def test_operator_follows_the_restatement(hip, n_vocab):
    x = cases.rows(n_vocab)
    ks, temps, streams, pos, mus = cases.requests(n_vocab)
    xb, stride = upload(hip, x, 5)                                          # poisoned padding between the rows
    ids, after, info = hip.sample_rows_miro(xb, cases.ROWS, n_vocab, stride, ks, temps, cases.SEED, streams, pos, mus, TAU, ETA)
    assert (after == -1).all()
    near = excused = proper = 0
    for r in range(cases.ROWS):
        a, b = check_row(x[r], int(ks[r]), float(temps[r]), int(mus[r]), cases.SEED, int(streams[r]), int(pos[r]), int(ids[r]), info[r],
                         f"vocab {n_vocab} row {r}")
        near += a
        excused += b
        proper += 1 < info[r]["n_keep"] < info[r]["n_cand"]
    print(f"vocab {n_vocab}: {near} near rows, {excused} excused draws, {proper} proper cuts of {cases.ROWS}")
    assert excused <= max(1, cases.ROWS // 1000)
    # the ids do not depend on whether the info is asked for
    again, _, none = hip.sample_rows_miro(xb, cases.ROWS, n_vocab, stride, ks, temps, cases.SEED, streams, pos, mus, TAU, ETA, info=False)
    assert none is None and again.tolist() == ids.tolist()


# ------------------------------------------------------------------------------------------------------------ 2. edges

@pytest.mark.parametrize("n", [1000, 3000])
def test_an_all_equal_row_keeps_everything_or_the_first_as_mu_crosses(hip, n):
    """every mass is 2^36 exactly, here and on the device: the cut keeps all n ids while mu >= lg16(n 2^36) - lg16(2^36) and the first
    alone one unit below"""
    xb = upload(hip, np.full(n, 1.5, np.float32), 3)[0]
    cross = ref.lg16(n << 36) - ref.lg16(1 << 36)
    streams = np.arange(64)
    for mu, want in ((cross, n), (cross + 1, n), (cross - 1, 1), (0, 1), (ref.MU_MAX, n), (-ref.MU_MAX, 1)):
        ids, _, info = hip.sample_rows_miro(xb, 64, n, 0, n, 1.0, 5, streams, 9, mu, TAU, ETA)
        assert (info["n_keep"] == want).all() and (info["n_cand"] == n).all() and (info["Z"] == n << 36).all(), (mu, info[0])
        assert (info["Zk"] == want << 36).all() and (info["q_id"] == 1 << 36).all()
        s = ref.lg16(want << 36) - (36 << 16)
        assert (info["s"] == s).all() and (info["mu_next"] == ref.update(mu, s, TAU_Q, ETA_Q)).all(), (mu, info[0])
        if want == 1:
            assert (ids == 0).all()                                          # the first of C: the lowest index among the maxima
        else:
            assert (ids >= 0).all() and (ids < n).all() and len(set(ids.tolist())) > 16     # ... and the draw spreads over them
    # top_k cuts the run first: the candidates are the lowest indices, the crossing is theirs
    for k in (300, 2 * n // 3):
        cross_k = ref.lg16(k << 36) - (36 << 16)
        ids, _, info = hip.sample_rows_miro(xb, 64, n, 0, k, 0.7, 5, streams, 9, cross_k, TAU, ETA)
        assert (info["n_cand"] == k).all() and (info["n_keep"] == k).all() and (ids < k).all(), k
        ids, _, info = hip.sample_rows_miro(xb, 64, n, 0, k, 0.7, 5, streams, 9, cross_k - 1, TAU, ETA)
        assert (info["n_keep"] == 1).all() and (ids == 0).all(), k


@pytest.mark.parametrize("n_vocab", [1500, 32003])
def test_both_sides_of_the_candidate_count_at_which_the_routine_changes(hip, n_vocab):
    """the same contract at 1023 / 1024 / 1025 candidates, on distinct values and on a grid whose k-th value is a run of equals"""
    r = np.random.default_rng(n_vocab)
    x = (r.standard_normal((2, n_vocab)) * 3.0).astype(np.float32)
    x[1] = (np.round(x[1] * 4.0) / 4.0).astype(np.float32)
    xb, stride = upload(hip, x, 3)
    lengths = {}
    for k in (1023, 1024, 1025):
        for mu_bits in (3, 6, 9, 40):
            ids, _, info = hip.sample_rows_miro(xb, 2, n_vocab, stride, k, 1.0, 31, [4, 9], 17, mu_bits << 16, TAU, ETA)
            for q in range(2):
                check_row(x[q], k, 1.0, mu_bits << 16, 31, (4, 9)[q], 17, int(ids[q]), info[q], f"vocab {n_vocab} k {k} mu {mu_bits} row {q}")
                lengths.setdefault((mu_bits, q), []).append(int(info[q]["n_keep"]))
    # one more candidate at the tail of the order changes little: the kept lengths on the two sides are neighbours
    assert all(max(v) - min(v) <= 2 for v in lengths.values()), lengths
    assert any(1 < v[0] < 1023 for v in lengths.values())


@pytest.mark.parametrize("n", [1000, 32003])
def test_a_bias_table_that_bans_all_but_three_ids(hip, n):
    r = np.random.default_rng(12)
    x = (r.standard_normal((8, n)) * 3.0).astype(np.float32)
    open_ids = [17, 500, 999]
    b = bref.table(n, allow=open_ids)
    xb, stride = upload(hip, x, 2)
    bb = upload(hip, b)[0]
    for k in (40, n):                                                       # (k = n: every -inf entry is a candidate, with no mass)
        for mu_bits in (0, 1, 4, 40):
            ids, _, info = hip.sample_rows_miro(xb, 8, n, stride, k, 0.9, 77, np.arange(8), 11, mu_bits << 16, TAU, ETA, bias=bb, bias_stride=0)
            assert np.isin(ids, open_ids).all()
            for q in range(8):
                check_row(bref.biased(x[q], b), k, 0.9, mu_bits << 16, 77, q, 11, int(ids[q]), info[q], f"banned k={k} mu={mu_bits} row {q}")
                assert info[q]["n_cand"] == k and 1 <= info[q]["n_keep"] <= 3
    # the same rows with the table as bias row r of a stack
    ids2, _, info2 = hip.sample_rows_miro(xb, 8, n, stride, n, 0.9, 77, np.arange(8), 11, 40 << 16, TAU, ETA, bias=upload(hip, np.tile(b, (8, 1)))[0],
                                          bias_stride=n)
    assert ids2.tolist() == ids.tolist() and info2.tobytes() == info.tobytes()


@pytest.mark.parametrize("n", [1000, 3000])
def test_a_masked_state_a_final_one_and_a_penalty(hip, n):
    """state 0 allows every third id, state 1 is final, state 2 allows the upper half: the step is the restatement's on the row the mask
    leaves (the operator that writes that row out is the rung below's), the next state is the pool's entry, and the penalty comes first"""
    r = np.random.default_rng(n)
    x = (r.standard_normal((6, n)) * 3.0).astype(np.float32)
    ids_ = np.arange(n)
    nxt = np.full((3, n), 0xFFFF, np.uint16)
    nxt[0, ids_ % 3 == 0] = 2
    nxt[1, :] = 1
    nxt[2, ids_ >= n // 2] = np.where(ids_[ids_ >= n // 2] % 2 == 0, 0, 1)
    flags = np.array([0, 1, 0], np.uint8)
    pool = hip.fsm_upload(nxt, flags)
    states = [0, 1, 2, -1, 0, 2]
    hist = [list(range(0, 60, 3)) * 2, [], list(range(n // 2, n // 2 + 50)), [5, 5, 7], [], []]
    xb, stride = upload(hip, x, 4)
    for k in (40, n):
        for mu_bits in (2, 7, 40):
            y = hip.mask_rows_fsm(xb, 6, n, stride, pool, states, hist, 1.3, 0.2, 0.1)
            ids, after, info = hip.sample_rows_miro(xb, 6, n, stride, k, 0.8, 3, np.arange(6), 21, mu_bits << 16, TAU, ETA, pool=pool, states=states,
                                                    hist=hist, r=1.3, freq=0.2, pres=0.1)
            for q in range(6):
                check_row(y[q], k, 0.8, mu_bits << 16, 3, q, 21, int(ids[q]), info[q], f"masked n={n} k={k} mu={mu_bits} row {q}")
                s = states[q]
                assert after[q] == (int(nxt[s][ids[q]]) if s in (0, 2) else s), (q, after[q])
                assert s not in (0, 2) or nxt[s][ids[q]] != 0xFFFF
    assert not (y[3] == x[3]).all() and (y[1] == x[1]).all()               # (row 3 was penalised, the final row only carries its state)


@pytest.mark.parametrize("n_vocab", [64, 1000, 32003])
def test_tau_zero_is_the_routine_below_bit_for_bit(hip, n_vocab):
    x = cases.rows(n_vocab)
    ks, temps, streams, pos, mus = cases.requests(n_vocab)
    ks = ks.copy()
    ks[::7] = 0                                                              # greedy rows too
    xb, stride = upload(hip, x, 5)
    cut, _ = hip.sample_rows_cut(xb, cases.ROWS, n_vocab, stride, ks, temps, cases.SEED, streams, pos, 1.0, 0.0, info=False)
    for want_info in (False, True):
        ids, _, info = hip.sample_rows_miro(xb, cases.ROWS, n_vocab, stride, ks, temps, cases.SEED, streams, pos, mus, 0.0, ETA, info=want_info)
        assert ids.tolist() == cut.tolist(), want_info
    assert (info["mu_next"] == mus).all() and not info["Z"].any() and not info["n_keep"].any() and not info["s"].any()
    # a greedy row ignores Mirostat and carries its mu on
    ids, _, info = hip.sample_rows_miro(xb, cases.ROWS, n_vocab, stride, 0, 1.0, cases.SEED, streams, pos, mus, TAU, ETA)
    assert ids.tolist() == x.argmax(axis=1).tolist() and (info["mu_next"] == mus).all() and not info["Z"].any()
    # under a table: gten_hip_sample_rows_cut at (1, 0) under the same table
    b = np.zeros(n_vocab, np.float32)
    b[: n_vocab // 2] = NINF
    bb = upload(hip, b)[0]
    want, _ = hip.sample_rows_cut(xb, cases.ROWS, n_vocab, stride, ks, temps, cases.SEED, streams, pos, 1.0, 0.0, bias=bb, bias_stride=0, info=False)
    ids, _, _ = hip.sample_rows_miro(xb, cases.ROWS, n_vocab, stride, ks, temps, cases.SEED, streams, pos, mus, 0.0, ETA, bias=bb, bias_stride=0, info=False)
    assert ids.tolist() == want.tolist()
    # in a state, penalised: gten_hip_sample_rows_fsm at (1, 0); rows with tau 0 beside rows with tau 5 in one launch
    nxt = np.zeros((2, n_vocab), np.uint16)
    nxt[0, 1::2] = 0xFFFF
    pool = hip.fsm_upload(nxt, np.array([0, 1], np.uint8))
    states = np.arange(cases.ROWS) % 3 - 1                                   # -1, 0, 1 (final)
    hist = [[int(v) for v in x[q].argsort()[-3:]] for q in range(cases.ROWS)]
    want, after_w, _ = hip.sample_rows_fsm(xb, cases.ROWS, n_vocab, stride, pool, states, ks, temps, cases.SEED, streams, pos, hist, 1.2, 0.1, 0.0)
    taus = np.where(np.arange(cases.ROWS) % 2 == 0, 0.0, TAU).astype(np.float32)
    for want_info in (False, True):
        ids, after, info = hip.sample_rows_miro(xb, cases.ROWS, n_vocab, stride, ks, temps, cases.SEED, streams, pos, mus, taus, ETA, pool=pool, states=states,
                                                hist=hist, r=1.2, freq=0.1, pres=0.0, info=want_info)
        off = (taus == 0) | (ks == 0)
        assert ids[off].tolist() == want[off].tolist() and after[off].tolist() == after_w[off].tolist(), want_info
    assert info["Z"][~off].all() and not info["Z"][off].any()


def test_mu_at_its_bounds(hip):
    r = np.random.default_rng(4)
    for n in (700, 2500):
        x = (r.standard_normal((4, n)) * 3.0).astype(np.float32)
        xb, stride = upload(hip, x, 1)
        for mu in (ref.MU_MAX, -ref.MU_MAX):
            ids, _, info = hip.sample_rows_miro(xb, 4, n, stride, n, 1.0, 8, np.arange(4), 2, mu, 32.0, 1.0)
            for q in range(4):
                check_row(x[q], n, 1.0, mu, 8, q, 2, int(ids[q]), info[q], f"bounds n={n} mu={mu} row {q}", 32 << 16, 65536)
            if mu > 0:
                # every id with a mass is kept; tau 32 at eta 1 would push mu past the bound: it stays there
                assert (info["n_keep"] == [int((nref.masses(nref.scores(x[q], nref.order(x[q], n), 1.0)) >= 1).sum()) for q in range(4)]).all()
                assert (info["mu_next"] == ref.MU_MAX).all()
            else:
                assert (info["n_keep"] == 1).all() and (info["s"] == 0).all() and (ids == x.argmax(axis=1)).all()
                assert (info["mu_next"] == -ref.MU_MAX + (32 << 16)).all()
        # ... and the floor of a negative product: tau_q = 1, s = 0, eta_q = 2^16 - 1 -> (-(2^16 - 1)) >> 16 = -1, not 0
        ids, _, info = hip.sample_rows_miro(xb, 4, n, stride, n, 1.0, 8, np.arange(4), 2, -ref.MU_MAX + 10, 2.0 ** -16, 1.0 - 2.0 ** -16)
        assert (info["s"] == 0).all() and (info["mu_next"] == -ref.MU_MAX + 11).all()


def test_operator_argument_errors(hip):
    xb = upload(hip, np.zeros(64))[0]

    def rc(n_rows=1, n_vocab=16, top_k=40, temp=1.0, mu=0, tau=5.0, eta=0.1, **kw):
        return hip.sample_rows_miro(xb, n_rows, n_vocab, 16, top_k, temp, 0, 0, 1, mu, tau, eta, rc=True, **kw)
    assert rc() == 0 and rc(tau=32.0, eta=1.0) == 0 and rc(tau=0.0, eta=float("nan"), mu=1 << 30) == 0      # (tau 0: eta and mu are not looked at)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(tau=-1.0), dict(tau=32.5), dict(tau=nan), dict(tau=inf), dict(eta=0.0), dict(eta=-0.1), dict(eta=1.5), dict(eta=nan), dict(eta=inf),
                dict(mu=ref.MU_MAX + 1), dict(mu=-ref.MU_MAX - 1), dict(top_k=-1), dict(temp=0.0), dict(temp=nan), dict(n_vocab=0), dict(n_vocab=65536)):
        assert rc(**bad) != 0, bad
    assert rc(top_k=0, temp=0.0) == 0 and rc(n_rows=0) == 0                  # greedy: the temperature is not looked at
    # a bias and a state on one row are refused; a bias beside unbound rows is not
    nxt = np.zeros((1, 16), np.uint16)
    pool = hip.fsm_upload(nxt, np.array([0], np.uint8))
    bb = upload(hip, np.zeros(16))[0]
    assert rc(pool=pool, states=0) == 0 and rc(bias=bb) == 0 and rc(pool=pool, states=-1, bias=bb) == 0
    assert rc(pool=pool, states=0, bias=bb) != 0 and rc(pool=pool, states=1) != 0 and rc(pool=pool, states=-2) != 0


# ------------------------------------------------------------------------------------------------------------ 3. independence

@pytest.mark.parametrize("n_vocab", [1000, 32003])
def test_results_do_not_depend_on_the_launch_shape(hip, n_vocab):
    """the same rows as one launch of 64 and as 64 launches of one, dense and with a stride past the row; and one row under 64
    requests (stride 0) against the same requests one by one: the same ids and the same info bytes"""
    x = cases.rows(n_vocab)
    ks, temps, streams, pos, mus = cases.requests(n_vocab)
    R = cases.ROWS
    dense, _ = upload(hip, x)
    padded, stride = upload(hip, x, 37)
    ids64, _, info64 = hip.sample_rows_miro(dense, R, n_vocab, n_vocab, ks, temps, cases.SEED, streams, pos, mus, TAU, ETA)
    idsp, _, infop = hip.sample_rows_miro(padded, R, n_vocab, stride, ks, temps, cases.SEED, streams, pos, mus, TAU, ETA)
    assert idsp.tolist() == ids64.tolist() and infop.tobytes() == info64.tobytes()
    one = [hip.sample_rows_miro(upload(hip, x[r])[0], 1, n_vocab, n_vocab, ks[r], temps[r], cases.SEED, streams[r], pos[r], mus[r], TAU, ETA) for r in range(R)]
    assert [int(i[0]) for i, _, _ in one] == ids64.tolist()
    assert b"".join(f.tobytes() for _, _, f in one) == info64.tobytes()
    row = upload(hip, x[3])[0]
    ids0, _, info0 = hip.sample_rows_miro(row, R, n_vocab, 0, ks, temps, cases.SEED, streams, pos, mus, TAU, ETA)
    one = [hip.sample_rows_miro(row, 1, n_vocab, 0, ks[r], temps[r], cases.SEED, streams[r], pos[r], mus[r], TAU, ETA) for r in range(R)]
    assert [int(i[0]) for i, _, _ in one] == ids0.tolist() and b"".join(f.tobytes() for _, _, f in one) == info0.tobytes()
    assert len(set(info0["n_keep"].tolist())) > 3                            # (the requests differ, so do the cuts)


# ------------------------------------------------------------------------------------------------------------ 4. the feedback chain

def test_feedback_chain_on_the_operator(hip):
    """tests/test_mirostat_cpu.py's chain with every step drawn by the operator, mu taken from each launch's mu_next: the same
    inequality"""
    rows = ref.chain_rows(400, 2048)
    tau_q, eta_q = ref.q16(3.0, 0.1)[1:]
    want, near = ref.chain(rows, 1.0, tau_q, eta_q, True)
    xb, stride = upload(hip, rows)
    V = rows.shape[1]
    out = {}
    for feedback in (True, False):
        mu, s = 2 * tau_q, []
        for i in range(len(rows)):
            _, _, info = hip.sample_rows_miro(xb.view(4 * i * stride), 1, V, stride, V, 1.0, 77, 5, i + 1, mu, 3.0, 0.1)
            s.append(int(info[0]["s"]))
            assert int(info[0]["mu_next"]) == ref.update(mu, s[-1], tau_q, eta_q)
            if feedback:
                mu = int(info[0]["mu_next"])
        out[feedback] = s
    a, b = ref.miss(out[True], tau_q), ref.miss(out[False], tau_q)
    print(f"|mean s - tau| over the second half on the device: {a:.4f} bits with feedback, {b:.4f} at mu = 2 tau; restatement with feedback "
          f"{ref.miss(want, tau_q):.4f} (near steps: {near})")
    print(f"largest |s device - s restatement| over the chain with feedback: {max(abs(x - y) for x, y in zip(out[True], want))} (2^-16 bit)")
    assert a < b
