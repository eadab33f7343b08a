"""-m gpu: repetition, frequency and presence penalties on the device (include/gten_hip_penalty.h, include/gten_host_penalty.h,
DESIGN.md §3.14).

Everything here is an equality.  gten_hip_penalize_rows is held to tests/penalty_ref.py bit for bit; gten_hip_sample_rows_pen to the
EXISTING operators (sample_rows / sample_rows_biased / sample_rows_cut) given the restatement's penalised row as their logits and the
same table: the same id, and the same cut info bytes -- no near-tie excuse, because both sides run the same device code on the same
f32 row.  The decoder is held to the operator on its own steps' logits with the host's copy of the ids so far, the host paths to each
other.

Not tested: the refusal of a decoder whose max_ctx >= 65535.  No such decoder can be created (the RoPE table ends at 2048 positions),
so the check in gten_hip_decoder_set_penalty cannot be reached from outside."""
import numpy as np
import pytest

import bias_ref as bref
import penalty_ref as ref
from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from test_bias_gpu import NINF, SEED, Dec, P, upload
from test_logprobs_gpu import bits, dec_ask, dec_records
from test_nucleus_gpu import dec_cut, model_setup

pytestmark = pytest.mark.gpu

VOCABS = [1, 2, 1023, 1024, 1025, 32003, 65535]    # an odd last half-word, both sides of the workgroup's width, the largest LDS
LENGTHS = [0, 1, 1023, 1024, 1025, 2048]           # window lengths: none, one, both sides of the workgroup's width, two trips
PENS = [(1.3, 0.0, 0.0), (0.7, 0.0, 0.0), (1.0, 0.25, 0.0), (1.0, 0.0, -0.5), (1.1, -0.125, 0.75), (8.0, 100.0, -100.0), (0.125, 0.03, 0.0)]
TOTAL = 24


def rows_of(n_vocab, n_rows, seed):
    """logits with every sign: positive, negative, +0 (i % 7 == 3) and -0 (i % 7 == 5)"""
    g = np.random.default_rng(seed)
    x = (g.standard_normal((n_rows, n_vocab)) * 3.0).astype(np.float32)
    i = np.arange(n_vocab)
    x[:, i % 7 == 3] = 0.0
    x[:, i % 7 == 5] = -0.0
    return x


def windows(n_vocab, seed):
    """one window per LENGTHS entry: random ids, with -1 and n_vocab among them (ignored), and in the long ones one id 300 times (a
    count above a byte, same-word atomics), the pairs 2j / 2j + 1 (both halves of a word) and the signed zeros' ids"""
    g = np.random.default_rng(seed)
    out = []
    for L in LENGTHS:
        ids = g.integers(0, n_vocab, L).astype(np.int32)
        if L >= 1023:
            hot = int(g.integers(0, n_vocab))
            ids[:300] = hot
            ids[300:340] = np.arange(40) % n_vocab
            ids[340:344] = np.array([3, 5, 10, 12]) % n_vocab
            ids[344], ids[345], ids[-1] = -1, n_vocab, n_vocab + 7
        out.append(ids)
    return out


def pens_for(n_rows, shift=0):
    p = [PENS[(r + shift) % len(PENS)] for r in range(n_rows)]
    return (np.array([v[0] for v in p], np.float32), np.array([v[1] for v in p], np.float32), np.array([v[2] for v in p], np.float32))


# ------------------------------------------------------------------------------------------------------------ 1. the row

@pytest.mark.parametrize("n_vocab", VOCABS)
def test_penalize_rows_equals_the_restatement_bit_for_bit(hip, n_vocab):
    hist = windows(n_vocab, 100 + n_vocab)
    R = len(hist)
    x = rows_of(n_vocab, R, n_vocab)
    xb, stride = upload(hip, x, 3)
    b = np.zeros(n_vocab, np.float32)
    b[:: 3] = 1.5
    b[n_vocab // 2] = NINF
    bb = upload(hip, b)[0]
    for shift in range(3):
        r, f, p = pens_for(R, shift)
        y = hip.penalize_rows(xb, R, n_vocab, stride, hist, r, f, p)
        yb = hip.penalize_rows(xb, R, n_vocab, stride, hist, r, f, p, bias=bb, bias_stride=0)
        for q in range(R):
            want = ref.row(x[q], hist[q], r[q], f[q], p[q])
            assert (bits(y[q]) == bits(want)).all(), (n_vocab, shift, q, np.flatnonzero(bits(y[q]) != bits(want))[:5])
            wantb = ref.row(x[q], hist[q], r[q], f[q], p[q], b)
            assert (bits(yb[q]) == bits(wantb)).all(), (n_vocab, shift, q)
            assert yb[q][n_vocab // 2] == NINF                                                      # a ban stays a ban
            if len(hist[q]) >= 1023:
                assert ref.counts(hist[q], n_vocab).max() >= 300 and (bits(want) != bits(x[q])).any()
    # (1, 0, 0): the row itself, whatever the window
    y = hip.penalize_rows(xb, R, n_vocab, stride, hist, 1.0, 0.0, 0.0)
    assert (bits(y) == bits(x)).all()
    # one window for every row (stride 0 logits): the same row R times
    y = hip.penalize_rows(upload(hip, x[0])[0], 3, n_vocab, 0, hist[-1], 1.3, 0.1, 0.2)
    assert (bits(y) == bits(ref.row(x[0], hist[-1], 1.3, 0.1, 0.2))[None, :]).all()


# ------------------------------------------------------------------------------------------------------------ 2. the draw

def existing_ids(hip, p_rows, ks, temps, seed, streams, pos, top_p, min_p, b=None):
    """the ids of the operators that exist without penalties, on the rows p as logits: (plain or biased ids, cut ids, cut info)"""
    R, V = p_rows.shape
    pb = upload(hip, p_rows)[0]
    if b is None:
        plain = hip.sample_rows(pb, R, V, V, ks, temps, seed, streams, pos)
        cut, info = hip.sample_rows_cut(pb, R, V, V, ks, temps, seed, streams, pos, top_p, min_p)
    else:
        bb = upload(hip, b)[0]
        plain = hip.sample_rows_biased(pb, bb, R, V, V, 0, ks, temps, seed, streams, pos)
        cut, info = hip.sample_rows_cut(pb, R, V, V, ks, temps, seed, streams, pos, top_p, min_p, bias=bb, bias_stride=0)
    return plain, cut, info


@pytest.mark.parametrize("n_vocab", VOCABS)
def test_sample_rows_pen_draws_what_the_existing_operators_draw_from_the_penalised_row(hip, n_vocab):
    hist = windows(n_vocab, 200 + n_vocab)
    R = len(hist)
    x = rows_of(n_vocab, R, 7 * n_vocab + 1)
    xb, stride = upload(hip, x, 5)
    g = np.random.default_rng(n_vocab)
    streams = g.integers(0, 1 << 32, R, dtype=np.uint64).astype(np.uint32)
    pos = g.integers(1, 1 << 20, R).astype(np.int32)
    temps = np.array([0.7, 1.0, 1.5, 0.9, 1.0, 2.0], np.float32)
    b = np.zeros(n_vocab, np.float32)
    b[1:: 2] = -0.75
    if n_vocab > 2:
        b[n_vocab // 3] = NINF
    bb = upload(hip, b)[0]
    # 0: greedy; 1, 40: top-k; both sides of the 1024-candidate limit of the cut's two routines; the whole vocabulary
    for k in [0, 1, 40, 1023, 1024, 1025, n_vocab]:
        if k > n_vocab + 9:
            continue
        ks = np.full(R, k, np.int32)
        for shift, (tp, mp) in enumerate([(1.0, 0.0), (0.9, 0.02), (0.5, 0.0)]):
            r, f, p = pens_for(R, shift + k)
            prow = np.stack([ref.row(x[q], hist[q], r[q], f[q], p[q]) for q in range(R)])
            plain, cut, info = existing_ids(hip, prow, ks, temps, SEED, streams, pos, tp, mp)
            got, ginfo = hip.sample_rows_pen(xb, R, n_vocab, stride, ks, temps, SEED, streams, pos, hist, r, f, p, tp, mp, info=True)
            assert got.tolist() == cut.tolist() and ginfo.tobytes() == info.tobytes(), (n_vocab, k, tp, mp)
            got2, none = hip.sample_rows_pen(xb, R, n_vocab, stride, ks, temps, SEED, streams, pos, hist, r, f, p, tp, mp)
            assert none is None and got2.tolist() == cut.tolist()
            if tp == 1.0 and mp == 0.0:
                assert got.tolist() == plain.tolist(), (n_vocab, k)
            plain, cut, info = existing_ids(hip, prow, ks, temps, SEED, streams, pos, tp, mp, b)
            got, ginfo = hip.sample_rows_pen(xb, R, n_vocab, stride, ks, temps, SEED, streams, pos, hist, r, f, p, tp, mp, bias=bb, bias_stride=0, info=True)
            assert got.tolist() == cut.tolist() and ginfo.tobytes() == info.tobytes(), (n_vocab, k, tp, mp, "table")
            if tp == 1.0 and mp == 0.0:
                assert got.tolist() == plain.tolist()
            if n_vocab > 2:
                assert (got != n_vocab // 3).all()
    # (1, 0, 0) on every row: today's operators on x itself
    ks = np.array([0, 1, 40, 40, n_vocab, 1025], np.int32)
    plain, cut, info = existing_ids(hip, x, ks, temps, SEED, streams, pos, 0.8, 0.01)
    got, ginfo = hip.sample_rows_pen(xb, R, n_vocab, stride, ks, temps, SEED, streams, pos, hist, 1.0, 0.0, 0.0, 0.8, 0.01, info=True)
    assert got.tolist() == cut.tolist() and ginfo.tobytes() == info.tobytes()
    got, _ = hip.sample_rows_pen(xb, R, n_vocab, stride, ks, temps, SEED, streams, pos, hist, 1.0, 0.0, 0.0)
    assert got.tolist() == plain.tolist()


def test_penalties_that_move_the_maximum_the_threshold_and_make_ties(hip):
    """hand-made rows of 64 logits (values on a grid of 1/8, so every penalised value is exact and the premises can be asserted)"""
    V = 64
    x = np.linspace(-2.0, 5.875, V).astype(np.float32)[::-1].copy()          # x[0] = 5.875 is the maximum, descending by 1/8
    xb = upload(hip, x)[0]
    streams, pos = np.arange(32, dtype=np.uint32), np.full(32, 9, np.int32)

    def both(hist, pen, k, tp=1.0, mp=0.0, b=None):
        p = ref.row(x, hist, *pen)
        bb = None if b is None else upload(hip, b)[0]
        want = existing_ids(hip, np.tile(p, (32, 1)), np.full(32, k, np.int32), np.full(32, 0.8, np.float32), SEED, streams, pos, tp, mp, b)
        got, info = hip.sample_rows_pen(xb, 32, V, 0, k, 0.8, SEED, streams, pos, hist, *pen, tp, mp, bias=bb, bias_stride=0, info=True)
        assert got.tolist() == want[1].tolist() and info.tobytes() == want[2].tobytes()
        return (p if b is None else bref.biased(p, b)), got

    # the argmax is penalised: mx moves to the runner-up, greedy and sampled
    p, got = both([0, 0], (2.0, 0.0, 0.0), 0)
    assert int(np.argmax(p)) == 1 and (got == 1).all() and p[0] == np.float32(5.875 / 2)
    p, got = both([0, 0], (2.0, 0.0, 0.0), 8)
    assert p.max() == x[1] and 0 not in got.tolist()                          # 2.9375 is below the 8th value, 4.875
    # a candidate pushed out across the k-th value, and one pulled in (a negative freq raises it)
    p, got = both([3], (1.0, 0.0, 4.0), 8)
    assert np.sort(p)[-8] == x[8] and 3 not in got.tolist() and p[3] < x[8]
    p, got = both([40, 40], (1.0, -4.0, 0.0), 8)
    assert p[40] == x[40] + 8.0 and p[40] > np.sort(p)[-8] and len(set(got.tolist())) > 1
    p1, got1 = both([40, 40], (1.0, -4.0, 0.0), 1)
    assert (got1 == int(np.argmax(p1))).all()
    # a tie made by the penalty: x[0] - 0.125 == x[1]; greedy takes the first maximum, top-k 1 the lower index
    p, got = both([0], (1.0, 0.0, 0.125), 0)
    assert p[0] == p[1] == p.max() and (got == 0).all()
    p, got = both([0], (1.0, 0.0, 0.125), 1)
    assert (got == 0).all()
    p, got = both([0], (1.0, 0.125, 0.125), 1)                                 # ... and 0.25: the tie is now between ids 1 and 0 below it
    assert p[0] == x[2] and (got == 1).all()
    # a banned penalised id stays banned, also when the penalty would have made it the maximum
    b = np.zeros(V, np.float32)
    b[40] = NINF
    p, got = both([40, 40, 40], (1.0, -5.0, 0.0), 8, b=b)
    assert p[40] == NINF and 40 not in got.tolist()
    p, got = both([40, 40, 40], (1.0, -5.0, 0.0), 0, b=b)
    assert (got == 0).all()
    # under a cut: the penalised maximum's mass decides the nucleus
    p, got = both([0, 0, 1], (4.0, 0.5, 0.0), V, 0.6, 0.05)
    assert int(np.argmax(p)) == 2


def test_results_do_not_depend_on_the_launch_shape(hip):
    V = 32003
    hist = windows(V, 77)
    R = len(hist)
    x = rows_of(V, R, 5)
    g = np.random.default_rng(1)
    streams, pos = g.integers(0, 1 << 32, R, dtype=np.uint64).astype(np.uint32), g.integers(1, 1 << 20, R).astype(np.int32)
    ks, temps = np.array([0, 40, 1024, 1025, V, 1], np.int32), np.full(R, 0.9, np.float32)
    r, f, p = pens_for(R)
    args = lambda o: (ks[o], temps[o], SEED, streams[o], pos[o], [hist[i] for i in o], r[o], f[o], p[o], 0.9, 0.01)      # noqa: E731
    o = np.arange(R)
    ids, info = hip.sample_rows_pen(upload(hip, x)[0], R, V, V, *args(o), info=True)
    rev = o[::-1].copy()
    padded, stride = upload(hip, x[rev], 37)
    ids_r, info_r = hip.sample_rows_pen(padded, R, V, stride, *args(rev), info=True)
    assert ids_r[::-1].tolist() == ids.tolist() and info_r[::-1].tobytes() == info.tobytes()
    for q in range(R):
        one, inf = hip.sample_rows_pen(upload(hip, x[q])[0], 1, V, V, *args(np.array([q])), info=True)
        assert int(one[0]) == int(ids[q]) and inf.tobytes() == info[q: q + 1].tobytes(), q
    y = hip.penalize_rows(upload(hip, x)[0], R, V, V, hist, r, f, p)
    y_r = hip.penalize_rows(padded, R, V, stride, [hist[i] for i in rev], r[rev], f[rev], p[rev])
    assert (bits(y_r[::-1]) == bits(y)).all()


def test_operator_argument_errors(hip):
    xb = upload(hip, np.zeros(64))[0]
    rc = lambda **kw: hip.sample_rows_pen_rc(xb, kw.pop("n_rows", 1), kw.pop("n_vocab", 16), 16, **kw)      # noqa: E731
    assert rc() == 0 and rc(r=0.125) == 0 and rc(r=8.0, freq=100.0, pres=-100.0) == 0 and rc(hist=[1, 2, -5, 99]) == 0
    for bad in (dict(r=0.12), dict(r=8.5), dict(r=0.0), dict(r=-1.5), dict(r=float("nan")), dict(r=float("inf")), dict(freq=100.5), dict(freq=float("nan")),
                dict(pres=-101.0), dict(pres=float("inf")), dict(top_k=-1), dict(temp=0.0), dict(n_vocab=0), dict(n_vocab=65536),
                dict(hist=[0] * 65536)):
        assert rc(**bad) != 0, {k: (v if k != "hist" else len(v)) for k, v in bad.items()}
    assert rc(hist=[0] * 65535) == 0                                         # the longest window a u16 count holds
    assert rc(n_rows=0) == 0 and rc(top_k=0, temp=0.0) == 0


# ------------------------------------------------------------------------------------------------------------ 3. the decoder

# per sequence, by kind = q % 6: (top_k [-1: the whole vocabulary], (r, freq, pres), last_n, count the prompt, (top_p, min_p), table, n_top)
KINDS = [(0, (1.0, 0.0, 0.0), 0, True, (1.0, 0.0), -1, -1),                  # plain greedy: today's ids
         (0, (1.3, 0.0, 0.0), 0, True, (1.0, 0.0), -1, 0),                   # penalised greedy
         (40, (1.1, 0.2, 0.1), 4, True, (1.0, 0.0), -1, -1),                 # a window shorter than the run
         (40, (0.8, -0.1, 0.3), 0, False, (0.9, 0.05), -1, 3),               # only generated ids; under a cut; records
         (40, (1.0, 0.0, 0.0), 0, True, (1.0, 0.0), -1, -1),                 # plain top-k: today's ids
         (-1, (1.2, 0.5, 0.0), 0, True, (0.95, 0.0), 1, 2)]                  # the whole vocabulary under a table and a cut


def kind_requests(n_seq, V, shift=0):
    kd = [KINDS[(q + shift) % 6] for q in range(n_seq)]
    return dict(ks=np.array([V if k[0] < 0 else k[0] for k in kd], np.int32), rep=np.array([k[1][0] for k in kd], np.float32),
                freq=np.array([k[1][1] for k in kd], np.float32), pres=np.array([k[1][2] for k in kd], np.float32),
                last_n=np.array([k[2] for k in kd], np.int32), count=[k[3] for k in kd], top_p=np.array([k[4][0] for k in kd], np.float32),
                min_p=np.array([k[4][1] for k in kd], np.float32), tables=np.array([k[5] for k in kd], np.int32), tops=np.array([k[6] for k in kd], np.int32))


def dec_pen(d, q, r, f, p, start=0, last_n=0):
    d.o.set_penalty(float(r), float(f), float(p), int(start), int(last_n)) if d.one else d.o.set_penalty(q, float(r), float(f), float(p), int(start), int(last_n))


def dec_pen_info(d):
    r, f, p, s, l, on = d.o.penalty_info()
    return np.atleast_1d(r), np.atleast_1d(f), np.atleast_1d(p), np.atleast_1d(s), np.atleast_1d(l), on


def generate_pen(d, prompts, total, rq, temps, streams, penalised=True):
    n = d.n
    rep, freq, pres = (rq["rep"], rq["freq"], rq["pres"]) if penalised else (np.ones(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32))
    if d.one:
        t = int(rq["tops"][0])
        out = d.o.generate_penalized(prompts[0], total, -1, int(rq["ks"][0]), float(temps[0]), SEED, int(streams[0]), float(rep[0]), float(freq[0]),
                                     float(pres[0]), int(rq["last_n"][0]), rq["count"][0], float(rq["top_p"][0]), float(rq["min_p"][0]),
                                     int(rq["tables"][0]), 0, t if t >= 0 else None)
        return [out[0] if t >= 0 else out]
    return d.o.generate_penalized(prompts, total, -1, rq["ks"], temps, SEED, streams, rep, freq, pres, rq["last_n"], rq["count"], rq["top_p"], rq["min_p"],
                                  rq["tables"], None, rq["tops"])[0]


def operator_pen_ids(hip, rows, hists, biases, rq, sel, temps, streams, n):
    """one draw per row of `rows` (the sequences sel) with gten_hip_sample_rows_pen, under biases[i] where it is not None"""
    rows = np.asarray(rows, np.float32)
    V = rows.shape[1]
    out = np.zeros(len(rows), np.int64)
    on = np.array([b is not None for b in biases])
    for mask in (on, ~on):
        if not mask.any():
            continue
        i = np.flatnonzero(mask)
        s = np.asarray(sel)[i]
        bias = upload(hip, np.stack([biases[j] for j in i]))[0] if mask is on else None
        out[i] = hip.sample_rows_pen(upload(hip, rows[i])[0], len(i), V, V, rq["ks"][s], temps[s], SEED, streams[s], np.full(len(i), n, np.int32),
                                     [hists[j] for j in i], rq["rep"][s], rq["freq"][s], rq["pres"][s], rq["top_p"][s], rq["min_p"][s], bias=bias,
                                     bias_stride=V if bias is not None else 0)[0]
    return out


@pytest.mark.parametrize("n_seq", [1, 2, 16, 256])
def test_decoder_follows_the_operator_on_its_own_logits(hip, n_seq):
    """the three step forms (1, 2-8, 16+) and, at 256, lanes 0 and 3 (the lane offset of the penalties and of the ids): the ids of
    free-running generation (four steps per graph replay: the window grows inside the graph) are, step by step, the operator's on the
    teacher-forced step's logits and the host's copy of the ids so far -- eager steps and captured single steps alternating"""
    host = load_package().load_host()
    cfg, weights = model_setup(host, 512)
    V = cfg.n_vocab
    d = Dec(host, cfg, weights, n_seq)
    assert not dec_pen_info(d)[5]
    prompts = [list(host.synthetic_tokens(P, seed=900 + q, n_vocab=V)) for q in range(n_seq)]
    streams = (np.arange(n_seq, dtype=np.uint32) * 5 + 2)
    temps = np.full(n_seq, 0.9, np.float32)
    banned = sorted({int(t) for p in prompts[:6] for t in p})[: V // 2]
    d.o.set_bias_table(1, [(j, NINF) for j in banned])
    table = bref.table(V, [(j, NINF) for j in banned])
    shifts = (1, 2, 3, 5) if n_seq == 1 else (0, 2, 4) if n_seq == 2 else (0,)   # every kind at every step form
    # the runs in which nobody has ever penalised: this decoder's graphs are the ones it always captured
    unpens = {shift: generate_pen(d, prompts, TOTAL, kind_requests(n_seq, V, shift), temps, streams, penalised=False) for shift in shifts}
    assert not dec_pen_info(d)[5]
    differed = 0
    for shift in shifts:
        rq = kind_requests(n_seq, V, shift)
        unpen = unpens[shift]
        got = generate_pen(d, prompts, TOTAL, rq, temps, streams)
        r, f, p, s, l, on = dec_pen_info(d)
        assert on and (r == 1.0).all() and not f.any() and not p.any() and not s.any() and not l.any()         # dropped afterwards
        again = generate_pen(d, prompts, TOTAL, rq, temps, streams, penalised=False)
        for q in range(n_seq):
            assert len(got[q]) == TOTAL and got[q][:P].tolist() == prompts[q]
            assert again[q].tolist() == unpen[q].tolist(), q                      # ... and the decoder that has the rung gives today's ids
            if (q + shift) % 6 in (0, 4):
                assert got[q].tolist() == unpen[q].tolist(), q                    # a sequence without a penalty beside penalised ones
            else:
                differed += got[q].tolist() != unpen[q].tolist()
        # teacher-forced with those ids
        check = list(range(n_seq)) if n_seq <= 16 else list(range(0, 12)) + list(range(n_seq - 12, n_seq))
        starts = np.array([0 if c else P for c in rq["count"]], np.int32)
        rows0 = {}
        for q in range(n_seq):
            d.request(q, int(rq["ks"][q]), 0.9, SEED, int(streams[q]))
            assert d.bind_rc(q, int(rq["tables"][q])) == 0
            dec_ask(d, q, rq["tops"][q])
            dec_cut(d, q, rq["top_p"][q], rq["min_p"][q])
            dec_pen(d, q, rq["rep"][q], rq["freq"][q], rq["pres"][q], starts[q], rq["last_n"][q])
            row = d.prefill(q, prompts[q])
            if q in check:
                rows0[q] = row
            d.begin(q, got[q])
        r, f, p, s, l, on = dec_pen_info(d)
        pen_on = np.array([ref.is_on(rq["rep"][q], rq["freq"][q], rq["pres"][q]) for q in range(n_seq)])
        assert (bits(r) == bits(rq["rep"])).all() and (bits(f) == bits(rq["freq"])).all() and (bits(p) == bits(rq["pres"])).all()
        assert (s[pen_on] == starts[pen_on]).all() and (l[pen_on] == rq["last_n"][pen_on]).all() and not s[~pen_on].any()
        d.request(0, int(rq["ks"][0]), 0.9, SEED, int(streams[0]))               # the other setters leave the penalty alone
        assert bits(dec_pen_info(d)[0][0]) == bits(rq["rep"][0])
        assert d.sampler_launches() >= 1
        bias_of = [table if rq["tables"][q] >= 0 else None for q in check]
        hist = lambda q, n: got[q][ref.window(n, int(starts[q]), int(rq["last_n"][q]))[0]: n]                  # noqa: E731
        first = operator_pen_ids(hip, [rows0[q] for q in check], [hist(q, P) for q in check], bias_of, rq, check, temps, streams, P)
        assert first.tolist() == [int(got[q][P]) for q in check]
        for n in range(P + 1, TOTAL):
            d.o.decode_step(n, use_graph=(n % 2 == 0))
            assert [d.result(q, n) for q in range(n_seq)] == [int(g[n]) for g in got], n
            rows = np.stack([d.logits(q) for q in check])
            ids = operator_pen_ids(hip, rows, [hist(q, n) for q in check], bias_of, rq, check, temps, streams, n)
            assert ids.tolist() == [int(got[q][n]) for q in check], n
            for i, q in enumerate(check):
                if rq["tops"][q] >= 0:
                    # the record: from the raw row and the committed id, whatever the id was drawn from
                    olp, oti, otl = hip.row_top_logprobs(upload(hip, rows[i])[0], 1, V, V, int(got[q][n]), int(rq["tops"][q]))
                    rlp, rti, rtl = dec_records(d, q, n, 1, int(rq["tops"][q]))
                    assert bits(rlp[0]) == bits(olp[0]) and rti[0].tolist() == oti[0].tolist() and (bits(rtl[0]) == bits(otl[0])).all(), (q, n)
            if n in (P + 2, TOTAL - 1):
                d.o.decode_step(n, use_graph=(n % 2 == 1))                         # a repeated step derives the same counts: the same ids
                assert [d.result(q, n) for q in range(n_seq)] == [int(g[n]) for g in got], n
        for q in range(n_seq):
            d.request(q, 0)
            assert d.bind_rc(q, -1) == 0
            dec_ask(d, q, -1)
            dec_cut(d, q, 1.0, 0.0)
            dec_pen(d, q, 1.0, 0.0, 0.0)
        assert d.sampler_launches() == 0 and dec_pen_info(d)[5]
    assert differed >= 1                                                     # the penalties changed something
    d.o.close()


def test_penalised_greedy_leaves_the_loop_where_the_restatement_says(hip):
    """plain greedy from a small model repeats itself; the restatement, run over the plain run's own logits, names the first step at
    which a penalty changes the id and the id it changes it to: penalised greedy equals plain greedy before it and takes that id there
    -- with the prompt counted (start 0) and with generated ids only (start = the prompt's length)"""
    host = load_package().load_host()
    cfg, weights = model_setup(host, 512, max_ctx=64)
    V, total = cfg.n_vocab, 48
    m = host.model(cfg)
    for i, w in enumerate(weights):
        m.set_weight(i, w)
    pen = (1.5, 0.0, 1.0)
    found = 0
    for seed in range(8):
        prompt = list(host.synthetic_tokens(P, seed=40 + seed, n_vocab=V))
        plain = m.generate_penalized(prompt, total)
        assert plain.tolist() == m.generate_biased(prompt, total).tolist()
        if len(set(plain[P:].tolist())) == total - P:
            continue                                                          # (this prompt does not repeat an id)
        rows = {P: m.logits(prompt, 0)}
        m.decode_begin(plain)
        for n in range(P + 1, total):
            m.decode_step(n)
            rows[n] = m.step_logits()
        for count_prompt in (True, False):
            want = next(((n, ref.greedy(ref.decoder_row(rows[n], plain, n, *pen, 0 if count_prompt else P, 0))) for n in range(P, total)
                         if ref.greedy(ref.decoder_row(rows[n], plain, n, *pen, 0 if count_prompt else P, 0)) != plain[n]), None)
            got = m.generate_penalized(prompt, total, rep=pen[0], freq=pen[1], pres=pen[2], count_prompt=count_prompt)
            if want is None:
                assert got.tolist() == plain.tolist(), (seed, count_prompt)
                continue
            n, tok = want
            assert got[:n].tolist() == plain[:n].tolist() and int(got[n]) == tok, (seed, count_prompt, n)
            found += 1
    assert found >= 2
    assert m.penalty_info()[:3] == (1.0, 0.0, 0.0)
    m.close()


def test_requests_are_checked_and_read_back(hip):
    pkg = load_package()
    host = pkg.load_host()
    cfg, weights = model_setup(host)
    d = Dec(host, cfg, weights, 2)
    for bad in ((0.12, 0, 0, 0, 0), (8.5, 0, 0, 0, 0), (float("nan"), 0, 0, 0, 0), (float("inf"), 0, 0, 0, 0), (-2.0, 0, 0, 0, 0), (1.1, 100.5, 0, 0, 0),
                (1.1, float("nan"), 0, 0, 0), (1.1, 0, -100.5, 0, 0), (1.1, 0, float("inf"), 0, 0), (1.1, 0, 0, -1, 0), (1.1, 0, 0, 0, -1)):
        assert d.o.set_penalty_rc(0, *bad) != 0, bad
    assert d.o.set_penalty_rc(2, 1.1) != 0 and d.o.set_penalty_rc(-1, 1.1) != 0
    assert not dec_pen_info(d)[5] and d.o.set_penalty_rc(1, 1.0, 0.0, 0.0, 5, 7) == 0 and not dec_pen_info(d)[5]   # clearing what was never set
    assert d.sampler_launches() == 0
    d.o.set_penalty(1, 1.25, -0.5, 2.0, 3, 9)
    r, f, p, s, l, on = dec_pen_info(d)
    assert on and r.tolist() == [1.0, 1.25] and f.tolist() == [0.0, -0.5] and p.tolist() == [0.0, 2.0] and s.tolist() == [0, 3] and l.tolist() == [0, 9]
    assert d.sampler_launches() >= 1                                         # a penalty moves a greedy id: the step ends in the sampler launch
    assert d.o.set_penalty_rc(1, 9.0) != 0 and dec_pen_info(d)[0].tolist() == [1.0, 1.25]      # a refused request leaves the one in force
    d.o.set_penalty(1)
    assert d.sampler_launches() == 0 and dec_pen_info(d)[0].tolist() == [1.0, 1.0]
    d.o.close()
    try:
        hip.set_decode_persistent(True)
    except pkg.GtenHipError:
        return
    try:
        m = host.model(cfg)
        assert m.set_penalty_rc(1.1) != 0 and m.set_penalty_rc(1.0) == 0
        m.close()
    finally:
        hip.set_decode_persistent(False)


# ------------------------------------------------------------------------------------------------------------ 4. the host paths

@pytest.mark.parametrize("n_seq", [2, 16])
def test_generate_batch_and_serve_agree_and_leave_no_penalty(hip, n_seq):
    """prompts of uneven lengths, each alone (2 slots: on a model; 16: by itself on a 16-sequence decoder), the first n_seq as a fixed batch, all of them through n_seq slots in 8-step
    slices with uneven budgets (slots are reused -- a later, shorter prompt finds a longer one's ids behind its own -- and repeat
    their last step inside a slice): the same ids and records per prompt, sampled and greedy penalised requests alike"""
    pkg = load_package()
    host = pkg.load_host()
    cfg, weights = model_setup(host, 512, max_ctx=96, seed=1618)
    V = cfg.n_vocab
    n = n_seq + 6
    lengths = [16 + (11 * j) % 40 for j in range(n)]
    prompts = [list(host.synthetic_tokens(L, seed=300 + j, n_vocab=V)) for j, L in enumerate(lengths)]
    total, seed, temp = 90, 13, 0.9
    max_new_each = [5 + (7 * j) % 16 for j in range(n)]
    ks = [(0, 40, V, 40, 0)[j % 5] for j in range(n)]
    rep = [(1.3, 1.1, 1.0, 0.9, 1.0)[j % 5] for j in range(n)]
    freq = [(0.0, 0.3, 0.0, -0.2, 0.0)[j % 5] for j in range(n)]
    pres = [(0.5, 0.0, 0.0, 0.4, 0.0)[j % 5] for j in range(n)]
    last_n = [(0, 8, 0, 20, 0)[j % 4] for j in range(n)]
    count = [bool(j % 3) for j in range(n)]
    top_p = [(1.0, 0.9, 0.8, 1.0, 1.0)[j % 5] for j in range(n)]
    tops = [(-1, 0, 3)[j % 3] for j in range(n)]
    m = host.model(cfg)
    for i, w in enumerate(weights):
        m.set_weight(i, w)
    wide = None
    if n_seq > 8:
        wide = host.batch(cfg, n_seq)
        for i, w in enumerate(weights):
            wide.set_weight(i, w)
    alone, plain = [], []
    for j, p in enumerate(prompts):
        L = len(p) + max_new_each[j]
        if wide is None:
            out = m.generate_penalized(p, L, -1, ks[j], temp, seed, j, rep[j], freq[j], pres[j], last_n[j], count[j], top_p[j], 0.0, -1, 0,
                                       tops[j] if tops[j] >= 0 else None)
            alone.append(out if tops[j] >= 0 else (out, None, None, None))
            plain.append(m.generate_nucleus(p, L, -1, ks[j], temp, seed, j, top_p[j], 0.0))
        else:
            # (16 sequences and more step in the wide forms, whose logits are not the single-sequence step's bit for bit: there
            #  "alone" is the prompt by itself on such a decoder -- in every slot, with its own stream)
            ids, lp, ti, tl = wide.generate_penalized([p] * n_seq, L, -1, ks[j], temp, seed, [j] * n_seq, rep[j], freq[j], pres[j], last_n[j], count[j],
                                                      top_p[j], 0.0, None, None, max(tops[j], 0))
            assert all(x.tolist() == ids[0].tolist() for x in ids)                                # (the slot does not matter)
            alone.append((ids[0], lp[0][: len(ids[0])], ti[0][: len(ids[0])], tl[0][: len(ids[0])]))
            plain.append(wide.generate_nucleus([p] * n_seq, L, -1, ks[j], temp, seed, [j] * n_seq, top_p[j], 0.0)[0])
    if wide is not None:
        assert (wide.penalty_info()[0] == 1.0).all()
        wide.close()
    assert m.penalty_info()[:5] == (1.0, 0.0, 0.0, 0, 0)
    assert sum(a[0].tolist() != q.tolist() for a, q in zip(alone, plain)) >= 2                      # the penalties changed something
    for j in range(n):
        if not ref.is_on(rep[j], freq[j], pres[j]):
            assert alone[j][0].tolist() == plain[j].tolist(), j
    # a first id that is the eos ends the answer before it, penalised or not
    j0 = next(j for j in range(n) if ref.is_on(rep[j], freq[j], pres[j]))
    eos = int(m.generate_penalized(prompts[j0], lengths[j0] + 1, -1, ks[j0], temp, seed, j0, rep[j0], freq[j0], pres[j0], last_n[j0], count[j0],
                                   top_p[j0])[lengths[j0]])
    cut =m.generate_penalized(prompts[j0], total, eos, ks[j0], temp, seed, j0, rep[j0], freq[j0], pres[j0], last_n[j0], count[j0], top_p[j0])
    assert cut.tolist() == prompts[j0]
    with pytest.raises(pkg.GtenHipError):
        m.generate_penalized(prompts[0], 40, -1, 40, temp, seed, 0, 9.0)
    assert m.penalty_info()[:3] == (1.0, 0.0, 0.0)
    m.close()
    b = host.batch(cfg, n_seq)
    for i, w in enumerate(weights):
        b.set_weight(i, w)
    first = list(range(n_seq))
    pick = lambda v: [v[j] for j in first]                                                            # noqa: E731
    ids, lp, ti, tl = b.generate_penalized(pick(prompts), total, -1, pick(ks), temp, seed, first, pick(rep), pick(freq), pick(pres), pick(last_n),
                                           pick(count), pick(top_p), 0.0, None, None, pick(tops))
    for j in first:
        L = len(alone[j][0])
        assert ids[j][:L].tolist() == alone[j][0].tolist(), j
        if tops[j] >= 0:
            assert (bits(lp[j][:L]) == bits(alone[j][1])).all() and ti[j][:L, : tops[j]].tolist() == alone[j][2].tolist(), j
    r, f, p, s, l, on = b.penalty_info()
    assert on and (r == 1.0).all() and not f.any() and not p.any() and not s.any() and not l.any()
    for sched in (1, 3):
        b.set_serve_schedule(sched)
        got, st, lp, ti, tl = b.serve_penalized(prompts, total, -1, ks, temp, seed, rep, freq, pres, last_n, count, top_p, 0.0, None, None, tops,
                                                slice_steps=8, max_new_each=max_new_each)
        assert st["admissions"] == n
        for j in range(n):
            L = len(got[j])
            assert got[j].tolist() == alone[j][0].tolist(), (sched, j)
            if tops[j] >= 0:
                assert (bits(lp[j][:L]) == bits(alone[j][1])).all() and ti[j][:L, : tops[j]].tolist() == alone[j][2].tolist(), (sched, j)
        r, f, p, s, l, _ = b.penalty_info()
        assert (r == 1.0).all() and not f.any() and not p.any() and not s.any() and not l.any()
    b.set_serve_schedule(0)
    with pytest.raises(pkg.GtenHipError):
        b.generate_penalized(pick(prompts), total, -1, 40, temp, seed, first, [1.1] * (n_seq - 1) + [0.01])
    with pytest.raises(pkg.GtenHipError):
        b.serve_penalized(prompts, total, -1, 40, temp, seed, 1.1, float("nan"))
    assert (b.penalty_info()[0] == 1.0).all()
    # the next plain call gives what a batch that never penalised gives
    after = b.generate_nucleus(pick(prompts), total, -1, pick(ks), temp, seed, first, pick(top_p), 0.0)
    b.close()
    fresh = host.batch(cfg, n_seq)
    for i, w in enumerate(weights):
        fresh.set_weight(i, w)
    want = fresh.generate_nucleus(pick(prompts), total, -1, pick(ks), temp, seed, first, pick(top_p), 0.0)
    assert not fresh.penalty_info()[5] and all(x.tolist() == y.tolist() for x, y in zip(after, want))
    fresh.close()


def test_cli_penalty_flags_print_the_ids_of_generate_penalized(hip, tmp_path):
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
    plain = m.generate_topk(prompt, n_pred, 32002, 40, 0.9, 7)
    want = m.generate_penalized(prompt, n_pred, 32002, 40, 0.9, 7, 0, 1.3, 0.2, 0.1, 8)
    want_greedy = m.generate_penalized(prompt, n_pred, 32002, 0, 0.9, 7, 0, 1.5, 0.0, 1.0)
    greedy = m.generate_biased(prompt, n_pred, 32002)
    m.close()
    assert want.tolist() != plain.tolist() or want_greedy.tolist() != greedy.tolist()
    common = [pkg.build.HOST_CLI, "-q4", "--ids", "--npred", str(n_pred), "--model", ckpt, "--tokenizer", vocab, "-p", "hello world", "--seed", "7", "--temp", "0.9"]
    r = subprocess.run(common + ["--topk", "40", "--repeat-penalty", "1.3", "--frequency-penalty", "0.2", "--presence-penalty", "0.1", "--repeat-last-n", "8"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [int(v) for v in r.stdout.split()] == want[len(prompt):].tolist()
    r = subprocess.run(common + ["-greedy", "--repeat-penalty", "1.5", "--presence-penalty", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [int(v) for v in r.stdout.split()] == want_greedy[len(prompt):].tolist()
