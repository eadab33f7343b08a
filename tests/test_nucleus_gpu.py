"""-m gpu: top-p and min-p truncation of the draw on the device, as exact integer cuts (include/gten_hip_nucleus.h,
include/gten_host_nucleus.h).

The operator is held to tests/nucleus_ref.py: n_cand and n_minp exactly, Z within delta = 2^-21 Z + 2 |C| (expf's error: the
restatement's masses come from float64 exp), n_nucleus delta-consistent on every row and EQUAL where the cut is clear of every prefix
sum by more than delta (tests/test_nucleus_cpu.py asserts that this is at least 90 % of the rows), and the id to the restatement's
draw over the device's own n_keep (tests/test_sampler_gpu.py's near-tie excuse only).  The decoder is held to the operator on its own
steps' logits, the host paths to each other."""
import numpy as np
import pytest

import bias_ref as bref
import nucleus_cases as cases
import nucleus_ref as ref
import sample_ref as sref
from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from helpers import Q4, Q8, tiny_config
from test_bias_gpu import NINF, SEED, TOTAL, Dec, P, upload
from test_model_gpu import host_cfg
from test_logprobs_gpu import bits, dec_ask, dec_records

pytestmark = pytest.mark.gpu

NEAR = 1e-4                                         # tests/test_sampler_gpu.py's near tie of two scores
LIMIT = 1024                                        # up to this many candidates smp_row_cut works on the candidates compacted into LDS,
                                                    # above it on the row with the mass histogram: every edge is run on both sides


def model_setup(host, n_vocab=512, max_ctx=64, seed=4711):
    cfg = host_cfg(tiny_config(Q4, Q8, n_vocab=n_vocab, n_heads=4, n_kv_heads=2, max_ctx=max_ctx))
    return cfg, [host.synth_weight(cfg, seed, i) for i in range(len(cfg.weight_shapes()))]


def check_row(y, k, temp, top_p, min_p, seed, stream, pos, got_id, info, what):
    """one row of the operator against the restatement; returns (the row is near, the id needed the near-tie excuse)"""
    c = ref.Cut(y, k, temp, top_p, min_p)
    Z, n_cand, n_nuc, n_minp, n_keep = int(info["Z"]), int(info["n_cand"]), int(info["n_nucleus"]), int(info["n_minp"]), int(info["n_keep"])
    print(f"{what}: Z dev {Z} ref {c.Z} (diff {Z - c.Z}, delta {c.delta:.0f}) n_cand {n_cand} n_nucleus dev {n_nuc} ref {c.n_nucleus} "
          f"n_minp dev {n_minp} ref {c.n_minp} near {bool(c.near)}")
    assert n_cand == c.n_cand and n_minp == c.n_minp, what
    assert abs(Z - c.Z) <= c.delta, (what, Z, c.Z, c.delta)
    assert c.consistent(n_nuc), (what, n_nuc, c.n_nucleus)
    if not c.near:
        assert n_nuc == c.n_nucleus, (what, n_nuc, c.n_nucleus)
    assert n_keep == min(n_nuc, n_minp) and n_keep >= 1, what
    want, _ = ref.draw(y, k, temp, seed, stream, pos, n_keep)
    excused = False
    if got_id != want:
        assert got_id in ref.order(y, k)[:n_keep].tolist(), (what, got_id)
        gap = sref.score_of(y, want, temp, seed, stream, pos) - sref.score_of(y, got_id, temp, seed, stream, pos)
        assert 0.0 <= gap <= NEAR, (what, got_id, want, gap)
        excused = True
    return bool(c.near), excused


# ------------------------------------------------------------------------------------------------------------ 1. the operator

@pytest.mark.parametrize("n_vocab", cases.VOCABS)
def test_operator_follows_the_restatement(hip, n_vocab):
    x = cases.rows(n_vocab)
    ks, temps, top_p, min_p, streams, pos = cases.requests(n_vocab)
    xb, stride = upload(hip, x, 5)                                          # poisoned padding between the rows
    ids, info = hip.sample_rows_cut(xb, cases.ROWS, n_vocab, stride, ks, temps, cases.SEED, streams, pos, top_p, min_p)
    near = excused = 0
    for r in range(cases.ROWS):
        a, b = check_row(x[r], int(ks[r]), float(temps[r]), float(top_p[r]), float(min_p[r]), cases.SEED, int(streams[r]), int(pos[r]), int(ids[r]),
                         info[r], f"vocab {n_vocab} row {r}")
        near += a
        excused += b
    print(f"vocab {n_vocab}: {near} near rows, {excused} excused draws of {cases.ROWS}")
    assert excused <= max(1, cases.ROWS // 1000)
    # the ids do not depend on whether the info is asked for
    again, none = hip.sample_rows_cut(xb, cases.ROWS, n_vocab, stride, ks, temps, cases.SEED, streams, pos, top_p, min_p, info=False)
    assert none is None and again.tolist() == ids.tolist()


# ------------------------------------------------------------------------------------------------------------ 2. ties and edges

@pytest.mark.parametrize("n", [1000, 3000])
def test_an_all_equal_row_keeps_the_first_indices_exactly(hip, n):
    xb = upload(hip, np.full(n, 1.5, np.float32), 3)[0]
    for p in (0.05, 0.25, 0.5, 0.9, 0.999):
        want = int(np.ceil(np.float64(np.float32(p)) * n))
        ids, info = hip.sample_rows_cut(xb, 64, n, 0, n, 1.0, 5, np.arange(64), 9, p, 0.0)
        assert (info["n_nucleus"] == want).all() and (info["Z"] == n << ref.MASS_BITS).all() and (info["n_keep"] == want).all(), (p, info[0])
        assert (ids >= 0).all() and (ids < want).all(), (p, ids)
        assert len(set(ids.tolist())) > min(want, 64) // 4                  # ... and the draw spreads over them
    # top_k cuts the run first: the nucleus is a share of the candidates
    for k in (300, 2 * n // 3):
        ids, info = hip.sample_rows_cut(xb, 64, n, 0, k, 0.7, 5, np.arange(64), 9, 0.5, 0.0)
        assert (info["n_cand"] == k).all() and (info["n_nucleus"] == k // 2).all() and (ids < k // 2).all(), k
    # min_p 1 keeps every maximum
    ids, info = hip.sample_rows_cut(xb, 8, n, 0, n, 1.0, 5, np.arange(8), 9, 1.0, 1.0)
    assert (info["n_minp"] == n).all() and (info["n_nucleus"] == n).all()


@pytest.mark.parametrize("n", [1000, 3000])
def test_a_long_run_of_equal_keys_across_the_cut_and_signed_zeros(hip, n):
    """seven ids in ten share the maximum (a run of more than 256 equal keys, spread over the row: the index select's two digits),
    once as 2.0 and once as -0 / +0 alternating: their masses are 2^36 exactly here and on the device"""
    run = np.flatnonzero(np.arange(n) % 10 < 7)
    for zeros in (False, True):
        y = np.full(n, -3.0 if not zeros else -1.0, np.float32)
        y[run] = np.where(np.arange(len(run)) % 2 == 0, -0.0, 0.0).astype(np.float32) if zeros else 2.0
        if zeros:
            assert np.signbit(y[run[0]]) and not np.signbit(y[run[1]])
        yb = upload(hip, y, 7)[0]
        for p in (0.4, 0.5, 0.8):
            c = ref.Cut(y, n, 1.0, p, 0.0)
            assert 256 < c.n_nucleus < len(run) and not c.near
            ids, info = hip.sample_rows_cut(yb, 64, n, 0, n, 1.0, 21, np.arange(64), 4, p, 0.0)
            assert (info["n_nucleus"] == c.n_nucleus).all() and (info["n_cand"] == n).all(), (zeros, p, info[0], c.n_nucleus)
            assert np.isin(ids, run[: c.n_nucleus]).all(), (zeros, p)
            for s in range(64):
                check_row(y, n, 1.0, p, 0.0, 21, s, 4, int(ids[s]), info[s], f"run zeros={zeros} p={p} stream {s}")
    # a value grid: the cut falls inside some run of equal keys below the maximum
    g = (np.round(np.random.default_rng(8).standard_normal(n) * 2.0) / 2.0).astype(np.float32)
    gb = upload(hip, g)[0]
    for p, k in ((0.5, n), (0.9, n), (0.9, 40), (0.99, 300), (0.99, 2 * n // 3)):
        ids, info = hip.sample_rows_cut(gb, 16, n, 0, k, 1.0, 21, np.arange(16), 4, p, 0.05)
        for s in range(16):
            check_row(g, k, 1.0, p, 0.05, 21, s, 4, int(ids[s]), info[s], f"grid p={p} k={k} stream {s}")


@pytest.mark.parametrize("n_vocab", [1500, 32003])
def test_both_sides_of_the_candidate_count_at_which_the_routine_changes(hip, n_vocab):
    """up to 1024 candidates the cut works on the candidates compacted into LDS, above on the row with the mass histogram: the same
    contract at 1023 / 1024 / 1025 candidates, on distinct values and on a grid whose k-th value is a run of equals"""
    r = np.random.default_rng(n_vocab)
    x = (r.standard_normal((2, n_vocab)) * 3.0).astype(np.float32)
    x[1] = (np.round(x[1] * 4.0) / 4.0).astype(np.float32)
    xb, stride = upload(hip, x, 3)
    lengths = {}
    for k in (1023, 1024, 1025):
        for p, m in ((0.9, 0.0), (0.99, 0.001), (1.0, 0.01)):
            ids, info = hip.sample_rows_cut(xb, 2, n_vocab, stride, k, 1.0, 31, [4, 9], 17, p, m)
            for q in range(2):
                check_row(x[q], k, 1.0, p, m, 31, (4, 9)[q], 17, int(ids[q]), info[q], f"vocab {n_vocab} k {k} p {p} m {m} row {q}")
                lengths.setdefault((p, m, q), []).append(int(info[q]["n_keep"]))
    # one more candidate at the tail of the order changes little: the kept lengths on the two sides are neighbours
    assert all(max(v) - min(v) <= 2 for v in lengths.values()), lengths


@pytest.mark.parametrize("n", [1000, 32003])
def test_a_bias_table_that_bans_all_but_three_ids(hip, n):
    r = np.random.default_rng(12)
    x = (r.standard_normal((8, n)) * 3.0).astype(np.float32)
    open_ids = [17, 500, 999]
    b = bref.table(n, allow=open_ids)
    xb, stride = upload(hip, x, 2)
    bb = upload(hip, b)[0]
    for k in (40, n):                                                       # (k = n: every -inf entry is a candidate, with no mass)
        for p, m in ((0.9, 0.0), (0.5, 0.0), (1.0, 0.3), (0.99, 0.01)):
            ids, info = hip.sample_rows_cut(xb, 8, n, stride, k, 0.9, 77, np.arange(8), 11, p, m, bias=bb, bias_stride=0)
            assert np.isin(ids, open_ids).all()
            for q in range(8):
                y = bref.biased(x[q], b)
                check_row(y, k, 0.9, p, m, 77, q, 11, int(ids[q]), info[q], f"banned k={k} p={p} m={m} row {q}")
                assert info[q]["n_cand"] == k and (info[q]["n_nucleus"] <= 3 or p == 1.0)
    # a finite table moves the cut as it moves the row
    fb = np.zeros(n, np.float32)
    fb[:10] = 8.0
    fb[10:20] = NINF
    ids, info = hip.sample_rows_cut(xb, 8, n, stride, n, 1.0, 77, np.arange(8), 11, 0.9, 0.0, bias=upload(hip, fb)[0], bias_stride=0)
    for q in range(8):
        check_row(bref.biased(x[q], fb), n, 1.0, 0.9, 0.0, 77, q, 11, int(ids[q]), info[q], f"finite table row {q}")


@pytest.mark.parametrize("n_vocab", [64, 1000, 32003])
def test_no_cut_is_the_plain_sampler_bit_for_bit(hip, n_vocab):
    x = cases.rows(n_vocab)
    ks, temps, _, _, streams, pos = cases.requests(n_vocab)
    ks = ks.copy()
    ks[::7] = 0                                                              # greedy rows too
    xb, stride = upload(hip, x, 5)
    plain = hip.sample_rows(xb, cases.ROWS, n_vocab, stride, ks, temps, cases.SEED, streams, pos)
    for want_info in (False, True):
        ids, info = hip.sample_rows_cut(xb, cases.ROWS, n_vocab, stride, ks, temps, cases.SEED, streams, pos, 1.0, 0.0, info=want_info)
        assert ids.tolist() == plain.tolist(), want_info
    assert (info["n_cand"] == np.minimum(ks, n_vocab)).all() and (info["n_keep"] == info["n_cand"]).all()
    assert not info["Z"][ks == 0].any() and (info["Z"][ks > 0] >= 1 << ref.MASS_BITS).all()        # greedy rows report nothing
    # a greedy row ignores a cut
    ids, _ = hip.sample_rows_cut(xb, cases.ROWS, n_vocab, stride, 0, 1.0, cases.SEED, streams, pos, 0.1, 0.9)
    assert ids.tolist() == x.argmax(axis=1).tolist()
    # under a table, no cut is gten_hip_sample_rows_biased
    b = np.zeros(n_vocab, np.float32)
    b[: n_vocab // 2] = NINF
    bb = upload(hip, b)[0]
    want = hip.sample_rows_biased(xb, bb, cases.ROWS, n_vocab, stride, 0, ks, temps, cases.SEED, streams, pos)
    ids, _ = hip.sample_rows_cut(xb, cases.ROWS, n_vocab, stride, ks, temps, cases.SEED, streams, pos, 1.0, 0.0, bias=bb, bias_stride=0, info=False)
    assert ids.tolist() == want.tolist()


def test_operator_argument_errors(hip):
    xb = upload(hip, np.zeros(64))[0]
    rc = lambda **kw: hip.sample_rows_cut_rc(xb, kw.pop("n_rows", 1), kw.pop("n_vocab", 16), 16, **kw)      # noqa: E731
    assert rc() == 0 and rc(top_p=1.0, min_p=1.0) == 0 and rc(top_p=1e-30, min_p=0.0) == 0
    for bad in (dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=1.0001), dict(top_p=float("nan")), dict(top_p=float("inf")),
                dict(min_p=-0.1), dict(min_p=1.5), dict(min_p=float("nan")), dict(min_p=float("inf")),
                dict(top_k=-1), dict(temp=0.0), dict(temp=float("nan")), dict(n_vocab=0), dict(n_vocab=65536)):
        assert rc(**bad) != 0, bad
    assert rc(top_k=0, temp=0.0, top_p=0.5) == 0                             # greedy: the temperature is not looked at
    assert rc(n_rows=0) == 0


# ------------------------------------------------------------------------------------------------------------ 3. independence

@pytest.mark.parametrize("n_vocab", [1000, 32003])
def test_results_do_not_depend_on_the_launch_shape(hip, n_vocab):
    """the same rows as one launch of 64 and as 64 launches of one, dense and with a stride past the row; and one row under 64
    requests (stride 0) against the same requests one by one: the same ids and the same info bytes"""
    x = cases.rows(n_vocab)
    ks, temps, top_p, min_p, streams, pos = cases.requests(n_vocab)
    R = cases.ROWS
    dense, _ = upload(hip, x)
    padded, stride = upload(hip, x, 37)
    ids64, info64 = hip.sample_rows_cut(dense, R, n_vocab, n_vocab, ks, temps, cases.SEED, streams, pos, top_p, min_p)
    idsp, infop = hip.sample_rows_cut(padded, R, n_vocab, stride, ks, temps, cases.SEED, streams, pos, top_p, min_p)
    assert idsp.tolist() == ids64.tolist() and infop.tobytes() == info64.tobytes()
    one = [hip.sample_rows_cut(upload(hip, x[r])[0], 1, n_vocab, n_vocab, ks[r], temps[r], cases.SEED, streams[r], pos[r], top_p[r], min_p[r]) for r in range(R)]
    assert [int(i[0]) for i, _ in one] == ids64.tolist()
    assert b"".join(f.tobytes() for _, f in one) == info64.tobytes()
    row = upload(hip, x[3])[0]
    ids0, info0 = hip.sample_rows_cut(row, R, n_vocab, 0, ks, temps, cases.SEED, streams, pos, top_p, min_p)
    one = [hip.sample_rows_cut(row, 1, n_vocab, 0, ks[r], temps[r], cases.SEED, streams[r], pos[r], top_p[r], min_p[r]) for r in range(R)]
    assert [int(i[0]) for i, _ in one] == ids0.tolist() and b"".join(f.tobytes() for _, f in one) == info0.tobytes()
    assert len(set(info0["n_nucleus"].tolist())) > 3                         # (the requests differ, so do the cuts)


# ------------------------------------------------------------------------------------------------------------ 4. the decoder

CUTS = {2: (0.9, 0.0), 3: (0.5, 0.05), 4: (0.3, 0.5), 5: (0.8, 0.1)}


def mixed(n_seq, shift, n_vocab):
    """per sequence, by kind = (q + shift) % 6: 0 greedy; 1 top-k 40; 2 top-k 40 under (0.9, 0); 3 the whole vocabulary under
    (0.5, 0.05); 4 greedy with a cut set (ignored); 5 under (0.8, 0.1) and table 1: top-k 40, or the whole vocabulary where that is
    more than LIMIT candidates (the row-wide routine under a table).  Some of kind 1 are bound too.  n_top cycles through -1 / 0 / 3."""
    kinds = [(q + shift) % 6 for q in range(n_seq)]
    ks = np.array([0 if kd in (0, 4) else n_vocab if kd == 3 or (kd == 5 and n_vocab > LIMIT) else 40 for kd in kinds], np.int32)
    top_p = np.array([CUTS.get(kd, (1.0, 0.0))[0] for kd in kinds], np.float32)
    min_p = np.array([CUTS.get(kd, (1.0, 0.0))[1] for kd in kinds], np.float32)
    tables = np.array([1 if kd == 5 or (kd == 1 and q % 4 == 1) else -1 for q, kd in enumerate(kinds)], np.int32)
    tops = np.array([(-1, 0, 3)[((q + shift) // 2) % 3] for q in range(n_seq)], np.int32)
    return kinds, ks, top_p, min_p, tables, tops


def dec_cut(d, q, top_p, min_p):
    d.o.set_cut(float(top_p), float(min_p)) if d.one else d.o.set_cut(q, float(top_p), float(min_p))


def dec_cut_info(d):
    a, b, t, on = d.o.cut_info()
    return np.atleast_1d(a), np.atleast_1d(b), np.atleast_1d(t), on


def dec_generate(d, prompts, total, ks, temps, seed, streams, tables, tops, top_p, min_p):
    """(ids per sequence, logprob [n][total], top_id [n][total][3], top_logprob) through generate_nucleus"""
    n = d.n
    lp, ti, tl = np.zeros((n, total), np.float32), np.full((n, total, 3), -1, np.int32), np.zeros((n, total, 3), np.float32)
    if d.one:
        t = int(tops[0])
        out = d.o.generate_nucleus(prompts[0], total, -1, int(ks[0]), float(temps[0]), seed, int(streams[0]), float(top_p[0]), float(min_p[0]),
                                   int(tables[0]), 0, t if t >= 0 else None)
        if t < 0:
            return [out], lp, ti, tl
        lp[0], ti[0, :, :t], tl[0, :, :t] = out[1], out[2], out[3]
        return [out[0]], lp, ti, tl
    ids, blp, bti, btl = d.o.generate_nucleus(prompts, total, -1, ks, temps, seed, streams, top_p, min_p, tables, None, tops)
    lp[:], ti[:, :, : bti.shape[2]], tl[:, :, : btl.shape[2]] = blp, bti, btl
    return ids, lp, ti, tl


def operator_cut_ids(hip, rows, biases, ks, temps, seed, streams, pos, top_p, min_p):
    """one draw per row with gten_hip_sample_rows_cut: under biases[r] where it is not None"""
    rows = np.asarray(rows, np.float32)
    out = np.zeros(len(rows), np.int64)
    on = np.array([bq is not None for bq in biases])
    V = rows.shape[1]
    if on.any():
        bs = np.stack([bq for bq in biases if bq is not None])
        out[on] = hip.sample_rows_cut(upload(hip, rows[on])[0], int(on.sum()), V, V, ks[on], temps[on], seed, streams[on], pos[on], top_p[on], min_p[on],
                                      bias=upload(hip, bs)[0], bias_stride=V, info=False)[0]
    if (~on).any():
        out[~on] = hip.sample_rows_cut(upload(hip, rows[~on])[0], int((~on).sum()), V, V, ks[~on], temps[~on], seed, streams[~on], pos[~on], top_p[~on],
                                       min_p[~on], info=False)[0]
    return out


@pytest.mark.parametrize("n_seq,n_vocab", [(1, 512), (2, 512), (16, 512), (128, 512), (1, 2048), (2, 2048), (16, 2048)])
def test_decoder_follows_the_operator_on_its_own_logits(hip, n_seq, n_vocab):
    """n_vocab 512: every cut runs on compacted candidates; 2048: the whole-vocabulary kinds run the row-wide routine, with and
    without a table, in k_dec_sample_cut at each step form's smallest width"""
    host = load_package().load_host()
    cfg, weights = model_setup(host, n_vocab)
    V = cfg.n_vocab
    d = Dec(host, cfg, weights, n_seq)
    assert d.sampler_launches() == 0 and not dec_cut_info(d)[3]
    prompts = [list(host.synthetic_tokens(P, seed=700 + q, n_vocab=V)) for q in range(n_seq)]
    streams = (np.arange(n_seq, dtype=np.uint32) * 3 + 1)
    temps = np.full(n_seq, 0.9, np.float32)
    zero, none = np.zeros(n_seq, np.int32), np.full(n_seq, -1, np.int32)
    ones, zeros_f = np.ones(n_seq, np.float32), np.zeros(n_seq, np.float32)
    greedy = d.generate(prompts, TOTAL, zero, temps, SEED, streams, none, zero)
    banned = sorted({int(g[p]) for g in greedy for p in (P, P + 1, P + 2)})[: V // 2]
    d.o.set_bias_table(1, [(j, NINF) for j in banned])
    table = bref.table(V, [(j, NINF) for j in banned])
    shifts = range(6) if n_seq == 1 else (0, 2, 4) if n_seq == 2 else (0,)
    # the runs in which nobody has ever set a cut: this decoder's graphs are the ones it always captured
    uncut = {s: d.generate(prompts, TOTAL, mixed(n_seq, s, V)[1], temps, SEED, streams, mixed(n_seq, s, V)[4], zero) for s in shifts}
    assert not dec_cut_info(d)[3]
    check = list(range(n_seq)) if n_seq <= 16 else [q for q in range(n_seq) if q % 16 < 6 or q >= n_seq - 6]
    differed, ever = 0, False
    for shift in shifts:
        kinds, ks, top_p, min_p, tables, tops = mixed(n_seq, shift, V)
        ever |= any(kd in (2, 3, 5) for kd in kinds)                                                 # (a greedy request's cut is not passed on by the host flows)
        got, lp, ti, tl = dec_generate(d, prompts, TOTAL, ks, temps, SEED, streams, tables, tops, top_p, min_p)
        a, b, _, on = dec_cut_info(d)
        assert (a == 1.0).all() and (b == 0.0).all()                                                 # the requests were dropped afterwards
        assert on == ever
        # the same requests with no cut anywhere, on the decoder that now launches the cut kernel
        base, blp, bti, btl = dec_generate(d, prompts, TOTAL, ks, temps, SEED, streams, tables, tops, ones, zeros_f)
        for q in range(n_seq):
            assert len(got[q]) == TOTAL and got[q][:P].tolist() == prompts[q]
            assert base[q].tolist() == uncut[shift][q].tolist(), (shift, q)                          # clearing restores the top-k ids
            if kinds[q] in (0, 1, 4):
                # no cut (or greedy): the ids of the run in which nobody set one, and the same record bytes
                assert got[q].tolist() == uncut[shift][q].tolist(), (shift, q, kinds[q])
                assert (bits(lp[q]) == bits(blp[q])).all() and ti[q].tolist() == bti[q].tolist() and (bits(tl[q]) == bits(btl[q])).all(), (shift, q)
            else:
                differed += got[q].tolist() != uncut[shift][q].tolist()
            if tables[q] >= 0:
                assert all(table[j] > NINF for j in got[q][P:]), (shift, q)
        # the host-driven loop, teacher-forced with those ids: every step's id against the operator on that step's logits
        rows0 = []
        for q in range(n_seq):
            d.request(q, int(ks[q]), 0.9, SEED, int(streams[q]))
            assert d.bind_rc(q, int(tables[q])) == 0
            dec_ask(d, q, tops[q])
            dec_cut(d, q, top_p[q], min_p[q])
            rows0.append(d.prefill(q, prompts[q]))
            d.begin(q, got[q])
        ever |= 4 in kinds                                                                           # (set directly, it is stored -- and ignored while greedy)
        a, b, t, on = dec_cut_info(d)
        assert on == ever and (bits(a) == bits(top_p)).all() and (bits(b) == bits(min_p)).all()
        assert (bits(t) == bits(np.array([ref.t_of(m) for m in min_p], np.float32))).all()
        d.request(0, int(ks[0]), 0.9, SEED, int(streams[0]))                                         # set_sampling leaves the cut alone
        assert bits(dec_cut_info(d)[0][0]) == bits(top_p[0])
        assert (d.sampler_launches() >= 1) == bool((ks > 0).any() or (tables >= 0).any() or (tops >= 0).any())
        bias_of = lambda q: table if tables[q] >= 0 else None                                        # noqa: E731
        first = operator_cut_ids(hip, rows0, [bias_of(q) for q in range(n_seq)], ks, temps, SEED, streams, np.full(n_seq, P, np.int32), top_p, min_p)
        assert first.tolist() == [int(g[P]) for g in got], shift
        asking = [q for q in check if tops[q] >= 0]
        for n in range(P + 1, TOTAL):
            d.o.decode_step(n)
            assert [d.result(q, n) for q in range(n_seq)] == [int(g[n]) for g in got], (shift, n)
            rows = np.stack([d.logits(q) for q in check])
            ids = operator_cut_ids(hip, rows, [bias_of(q) for q in check], ks[check], temps[check], SEED, streams[check], np.full(len(check), n, np.int32),
                                   top_p[check], min_p[check])
            assert ids.tolist() == [int(got[q][n]) for q in check], (shift, n)
            for q in asking:
                # the record: from the raw row and the committed id, whatever cut the id was drawn under
                olp, oti, otl = hip.row_top_logprobs(upload(hip, rows[check.index(q)])[0], 1, V, V, int(got[q][n]), int(tops[q]))
                rlp, rti, rtl = dec_records(d, q, n, 1, int(tops[q]))
                assert bits(rlp[0]) == bits(olp[0]) and rti[0].tolist() == oti[0].tolist() and (bits(rtl[0]) == bits(otl[0])).all(), (shift, q, n)
                assert bits(lp[q][n]) == bits(olp[0]) and ti[q][n][: tops[q]].tolist() == oti[0].tolist(), (shift, q, n)
            if n in (P + 3, TOTAL - 1):
                d.o.decode_step(n)                                                                   # a repeated step rewrites the same ids
                assert [d.result(q, n) for q in range(n_seq)] == [int(g[n]) for g in got], (shift, n)
        for q in range(n_seq):
            d.request(q, 0)
            assert d.bind_rc(q, -1) == 0
            dec_ask(d, q, -1)
            dec_cut(d, q, 1.0, 0.0)
        assert d.sampler_launches() == 0
    assert differed >= 1                                               # the cuts changed something
    again = d.generate(prompts, TOTAL, zero, temps, SEED, streams, none, zero)
    assert all(x.tolist() == g.tolist() for x, g in zip(again, greedy))
    d.o.close()


def test_requests_are_checked_and_read_back(hip):
    pkg = load_package()
    host = pkg.load_host()
    cfg, weights = model_setup(host)
    d = Dec(host, cfg, weights, 2)
    for bad in ((0.0, 0.0), (1.5, 0.0), (-1.0, 0.0), (float("nan"), 0.0), (0.9, -0.1), (0.9, 1.1), (0.9, float("nan")), (float("inf"), 0.0)):
        assert d.o.set_cut_rc(0, *bad) != 0, bad
    assert d.o.set_cut_rc(2, 0.9, 0.0) != 0 and d.o.set_cut_rc(-1, 0.9, 0.0) != 0
    assert not dec_cut_info(d)[3] and d.o.set_cut_rc(1, 1.0, 0.0) == 0 and not dec_cut_info(d)[3]       # clearing what was never set: nothing happens
    d.o.set_cut(1, 0.9, 0.25)
    a, b, t, on = dec_cut_info(d)
    assert on and a.tolist() == [1.0, np.float32(0.9)] and b.tolist() == [0.0, 0.25] and t[0] == NINF and bits(t[1]) == bits(ref.t_of(0.25))
    assert d.sampler_launches() == 0                                   # a cut alone samples nothing: the greedy graph
    d.o.set_sampling(1, 40, 0.9, 1, 2)
    assert d.sampler_launches() >= 1
    d.o.set_sampling(1, 0)
    d.o.close()
    # the persistent step has no sampler.  The product library is built without it and says so when asked; a build that has it
    # must refuse the cut on such a decoder.
    try:
        hip.set_decode_persistent(True)
    except pkg.GtenHipError:
        return
    try:
        m = host.model(cfg)
        assert m.set_cut_rc(0.9, 0.0) != 0 and m.set_cut_rc(1.0, 0.0) == 0
        m.close()
    finally:
        hip.set_decode_persistent(False)


# ------------------------------------------------------------------------------------------------------------ 5. the host paths

def test_generate_batch_and_serve_agree_and_leave_no_cut(hip):
    """10 prompts: each alone on a model, the first four as a batch of four, all of them through four slots with 8-step slices and
    uneven lengths (slots are reused and repeat their last step): the same ids and records per prompt; afterwards, and after a refused
    call, no sequence has a cut"""
    host = load_package().load_host()
    cfg, weights = model_setup(host, 2048, max_ctx=96, seed=1618)         # (2048 ids: the whole-vocabulary prompts take the row-wide routine)
    V = cfg.n_vocab
    n, n_seq = 10, 4
    lengths = [3 + (11 * j) % 40 for j in range(n)]
    prompts = [list(host.synthetic_tokens(L, seed=500 + j, n_vocab=V)) for j, L in enumerate(lengths)]
    total, seed, temp = 90, 13, 0.9
    max_new_each = [5 + (7 * j) % 16 for j in range(n)]
    ks = [0 if j % 5 == 4 else V if j % 5 == 3 else 40 for j in range(n)]
    top_p = [(0.9, 0.5, 1.0, 0.95, 0.7)[j % 5] for j in range(n)]
    min_p = [(0.0, 0.1, 0.0, 0.02, 0.0)[j % 5] for j in range(n)]
    tables = [(-1, 1)[(j // 2) % 2] for j in range(n)]
    tops = [(-1, 0, 3)[j % 3] for j in range(n)]
    allow = sorted(np.random.default_rng(9).choice(V, 64, replace=False).tolist())
    m = host.model(cfg)
    for i, w in enumerate(weights):
        m.set_weight(i, w)
    m.set_bias_table(1, allow=allow)
    alone, plain = [], []
    for j, p in enumerate(prompts):
        out = m.generate_nucleus(p, len(p) + max_new_each[j], -1, ks[j], temp, seed, j, top_p[j], min_p[j], tables[j], 0, tops[j] if tops[j] >= 0 else None)
        alone.append(out if tops[j] >= 0 else (out, None, None, None))
        plain.append(m.generate_biased(p, len(p) + max_new_each[j], -1, ks[j], temp, seed, j, tables[j], 0))
    assert m.cut_info()[:2] == (1.0, 0.0)
    assert sum(a[0].tolist() != p.tolist() for a, p in zip(alone, plain)) >= 2                       # the cuts changed something
    for j in range(n):
        if ks[j] == 0 or (top_p[j] == 1.0 and min_p[j] == 0.0):
            assert alone[j][0].tolist() == plain[j].tolist(), j
    with pytest.raises(load_package().GtenHipError):
        m.generate_nucleus(prompts[0], 40, -1, 40, temp, seed, 0, 1.5, 0.0)
    m.close()
    b = host.batch(cfg, n_seq)
    for i, w in enumerate(weights):
        b.set_weight(i, w)
    b.set_bias_table(1, allow=allow)
    first = list(range(n_seq))
    ids, lp, ti, tl = b.generate_nucleus([prompts[j] for j in first], total, -1, [ks[j] for j in first], temp, seed, first, [top_p[j] for j in first],
                                         [min_p[j] for j in first], [tables[j] for j in first], None, [tops[j] for j in first])
    for j in first:
        L = len(alone[j][0])
        assert ids[j][:L].tolist() == alone[j][0].tolist(), j
        if tops[j] >= 0:
            assert (bits(lp[j][:L]) == bits(alone[j][1])).all() and ti[j][:L, : tops[j]].tolist() == alone[j][2].tolist(), j
    a, c, _, on = b.cut_info()
    assert on and (a == 1.0).all() and (c == 0.0).all()
    for sched in (1, 3):
        b.set_serve_schedule(sched)
        got, st, lp, ti, tl = b.serve_nucleus(prompts, total, -1, ks, temp, seed, top_p, min_p, tables, None, tops, slice_steps=8, max_new_each=max_new_each)
        assert st["admissions"] == n
        for j in range(n):
            L = len(got[j])
            assert got[j].tolist() == alone[j][0].tolist(), (sched, j)
            if tops[j] >= 0:
                assert (bits(lp[j][:L]) == bits(alone[j][1])).all() and ti[j][:L, : tops[j]].tolist() == alone[j][2].tolist(), (sched, j)
                assert (bits(tl[j][:L, : tops[j]]) == bits(alone[j][3])).all(), (sched, j)
            else:
                assert not lp[j].any() and (ti[j] == -1).all()
        a, c, _, _ = b.cut_info()
        assert (a == 1.0).all() and (c == 0.0).all()
        ids_only, _ = b.serve_nucleus(prompts, total, -1, ks, temp, seed, top_p, min_p, tables, slice_steps=8, max_new_each=max_new_each)
        assert all(x.tolist() == y.tolist() for x, y in zip(ids_only, got))
    b.set_serve_schedule(0)
    # a refused request leaves no cut behind
    pkg = load_package()
    with pytest.raises(pkg.GtenHipError):
        b.generate_nucleus([prompts[j] for j in first], total, -1, 40, temp, seed, first, [0.9, 0.9, 0.9, 1.5], 0.0)
    with pytest.raises(pkg.GtenHipError):
        b.serve_nucleus(prompts, total, -1, 40, temp, seed, 0.9, -0.5)
    with pytest.raises(pkg.GtenHipError):
        b.generate_nucleus([prompts[j] for j in first], total, -1, 40, temp, seed, first, 0.9, 0.1, [99, -1, -1, -1])     # no such table
    a, c, _, _ = b.cut_info()
    assert (a == 1.0).all() and (c == 0.0).all()
    b.close()


def test_cli_top_p_prints_the_ids_of_generate_nucleus(hip, tmp_path):
    import subprocess
    from test_cli_gpu import write_vocab
    pkg = load_package()
    host = pkg.load_host()
    cfg = host.default_config(4, 3)
    ckpt, vocab = str(tmp_path / "tinyllama.q4.gten"), str(tmp_path / "vocab.bin")
    host.write_gten(cfg, 4242, ckpt)
    write_vocab(vocab)
    n_pred = 24
    prompt = host.tokenizer(vocab).encode("hello world")
    cfg.max_ctx = n_pred
    m = host.model(cfg)
    m.load_gten(ckpt)
    m.set_bias_table(0, [(200, NINF)])
    plain = m.generate_topk(prompt, n_pred, 32002, 40, 0.9, 7)
    want_cut = m.generate_nucleus(prompt, n_pred, 32002, 40, 0.9, 7, 0, 0.5, 0.1)
    want_all = m.generate_nucleus(prompt, n_pred, 32002, 32003, 0.9, 7, 0, 0.8, 0.0, 0, 0, 2)
    m.close()
    assert want_cut.tolist() != plain.tolist()
    common = [pkg.build.HOST_CLI, "-q4", "--ids", "--npred", str(n_pred), "--model", ckpt, "--tokenizer", vocab, "-p", "hello world", "--seed", "7", "--temp", "0.9"]
    r = subprocess.run(common + ["--topk", "40", "--top-p", "0.5", "--min-p", "0.1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [int(v) for v in r.stdout.split()] == want_cut[len(prompt):].tolist()
    r = subprocess.run(common + ["--topk", "32003", "--top-p", "0.8", "--ban", "200", "--logprobs", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    ids, lp, ti, tl = want_all
    assert [int(v) for v in lines[0].split()] == ids[len(prompt):].tolist() and len(lines) == 1 + len(ids) - len(prompt)
    for i, line in enumerate(lines[1:]):
        f = line.split()
        pos = len(prompt) + i
        assert int(f[0]) == ids[pos] and np.float32(f[1]) == lp[pos] and int(f[2].split(":")[0]) == ti[pos][0], (i, line)
