"""-m gpu: what the four host generation modes (greedy, top-k, bias tables, log-prob records) share above the C ABI -- the exits
that leave a call early, the state a call leaves behind, and the extras a call does not use.

Each mode sets up to three things on a decoder slot (sampling request, table binding, log-prob request) and has to take back
exactly those on every way out.  Held here, on a HostModel, a HostBatch of 2 and serve on 2 and 16 slots:
  * a call whose first id is the eos, or that has no room after the first id, returns the prompt (plus that id) with blank records;
  * after every call no sequence is bound, plain generate() gives the greedy ids it gave before anything was set, and a step
    the caller drives writes no record;
  * with no table and no log-prob request the three sampled entry points and the three sampled serves return the same ids, and
    with top_k 0 those are generate()'s and serve()'s."""
import numpy as np
import pytest

from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from test_bias_gpu import model_setup

pytestmark = pytest.mark.gpu

NINF = -np.inf
LENGTHS = [3, 5, 17, 20, 40]          # below and at or above 16: at 16 slots serve takes both prompt paths
TOTAL, MAX_NEW = 52, 10
K, TEMP, SEED = 40, 0.9, 77
N_TOP = 3
PAIRS = [(1, 0), (3, 2), (4, 3)]      # (longer, shorter) prompts of a 2-sequence batch: the longer one gets the early exit
KINDS = ["topk", "biased", "logprobs"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Env:
    pass


@pytest.fixture(scope="module")
def env(hip):
    e = Env()
    e.fresh = 0
    e.host = host = load_package().load_host()
    e.cfg, weights = model_setup(host, max_ctx=96, seed=2718)
    V = e.cfg.n_vocab
    e.prompts = [list(host.synthetic_tokens(L, seed=900 + L, n_vocab=V)) for L in LENGTHS]
    e.m, e.b2, e.b16 = host.model(e.cfg), host.batch(e.cfg, 2), host.batch(e.cfg, 16)
    for o in (e.m, e.b2, e.b16):
        for i, w in enumerate(weights):
            o.set_weight(i, w)
    # the greedy ids, before anything is set on any decoder
    e.greedy_m = [e.m.generate(p, TOTAL) for p in e.prompts]
    e.greedy_b2 = {pair: e.b2.generate([e.prompts[i] for i in pair], TOTAL) for pair in PAIRS}
    e.sixteen = [e.prompts[q % 5] for q in range(16)]
    e.greedy_b16 = e.b16.generate(e.sixteen, TOTAL)
    e.serve_greedy = {n: b.serve(e.prompts, TOTAL, -1, 4, MAX_NEW)[0] for n, b in ((2, e.b2), (16, e.b16))}
    # table 1 bans what greedy generation produces first: the constrained runs differ from the plain ones
    e.banned = sorted({int(g[len(p)]) for g, p in zip(e.greedy_m, e.prompts)} | {int(g[len(p) + 1]) for g, p in zip(e.greedy_m, e.prompts)})
    for o in (e.m, e.b2, e.b16):
        o.set_bias_table(1, [(j, NINF) for j in e.banned])
    # the record buffers exist (zeroed) from here on, and nobody asks
    e.m.set_logprobs(0)
    e.m.set_logprobs(-1)
    for b in (e.b2, e.b16):
        b.set_logprobs(0, 0)
        b.set_logprobs(0, -1)
    yield e
    for o in (e.m, e.b2, e.b16):
        o.close()


def model_call(m, kind, prompt, total, eos):
    """(ids, records or None) of one single-sequence call of `kind`"""
    if kind == "topk":
        return m.generate_topk(prompt, total, eos, K, TEMP, SEED, 5), None
    if kind == "biased":
        return m.generate_biased(prompt, total, eos, K, TEMP, SEED, 5, 1, 0), None
    ids, lp, ti, tl = m.generate_logprobs(prompt, total, N_TOP, eos, K, TEMP, SEED, 5, 1, 0)
    return ids, (lp, ti, tl)


def batch_call(b, kind, prompts, total, eos):
    """(ids per sequence, records [n_seq][total] or None) of one fixed-batch call of `kind`"""
    streams = [5, 6]
    if kind == "topk":
        return b.generate_topk(prompts, total, eos, K, TEMP, SEED, streams), None
    if kind == "biased":
        return b.generate_biased(prompts, total, eos, K, TEMP, SEED, streams, [1, 1], None), None
    ids, lp, ti, tl = b.generate_logprobs(prompts, total, N_TOP, eos, K, TEMP, SEED, streams, [1, 1], None)
    return ids, (lp, ti, tl)


def assert_blank(rec, sl=slice(None)):
    lp, ti, tl = rec
    assert not lp[sl].any() and (ti[sl] == -1).all() and not tl[sl].any()


def assert_same_records(got, want, n):
    """the first n positions of two record triples, bit for bit"""
    for g, w in zip(got, want):
        assert g[:n].shape == w[:n].shape
        assert (g[:n] == w[:n]).all() if g.dtype == np.int32 else (bits(g[:n]) == bits(w[:n])).all()


def no_record_written(e, read, ask, begin, step):
    """a step the caller drives on ids no call has seen leaves the record of its position as it was -- and writes one once the
    sequence asks (so the comparison can fail)"""
    n = 4
    e.fresh += 1
    begin(e.host.synthetic_tokens(n + 1, seed=5000 + e.fresh, n_vocab=e.cfg.n_vocab))
    before = read(n)
    step(n)
    assert_same_records(read(n), before, 1)
    ask(N_TOP)
    step(n)
    asked = read(n)
    ask(-1)
    assert asked[0][0] < 0 and (asked[1][0, :N_TOP] >= 0).all() and (asked[1][0, N_TOP:] == -1).all()
    assert (bits(asked[0]) != bits(before[0])).any() or (asked[1] != before[1]).any()


def clean_model(e, i):
    """the model after a call on prompt i: greedy as before, and no record from a step nobody asked about"""
    m = e.m
    assert m.generate(e.prompts[i], TOTAL).tolist() == e.greedy_m[i].tolist()
    no_record_written(e, lambda n: m.logprobs(n, 1, 20), m.set_logprobs, m.decode_begin, m.decode_step)
    assert m.generate(e.prompts[i], TOTAL).tolist() == e.greedy_m[i].tolist()


def clean_batch(e, b, prompts, greedy):
    """the batch after a call: nobody bound, greedy as before, no record from a step nobody asked about"""
    _, tb, un = b.bias_info()
    assert (tb == -1).all() and (un == 0).all()
    got = b.generate(prompts, TOTAL)
    assert all(g.tolist() == w.tolist() for g, w in zip(got, greedy))

    def begin(ids):
        for q in range(b.n_seq):
            b.decode_begin(q, ids)
    for q in (0, b.n_seq - 1):
        no_record_written(e, lambda n: b.logprobs(q, n, 1, 20), lambda t: b.set_logprobs(q, t), begin, b.decode_step)
    _, tb, un = b.bias_info()
    assert (tb == -1).all() and (un == 0).all()


@pytest.mark.parametrize("kind", KINDS)
def test_model_early_exits(env, kind):
    """first id == eos: the prompt alone; max_tokens == len(prompt) + 1: the prompt and that id, its record the full run's"""
    e = env
    for i, p in enumerate(e.prompts):
        P = len(p)
        full, full_rec = model_call(e.m, kind, p, TOTAL, -1)
        assert len(full) == TOTAL and full[:P].tolist() == p
        if kind != "topk":
            assert not set(full[P:].tolist()) & set(e.banned)
        ids, rec = model_call(e.m, kind, p, TOTAL, int(full[P]))
        assert ids.tolist() == p
        if rec:
            assert rec[0].shape == (P,) and rec[1].shape == (P, N_TOP)
            assert_blank(rec)
        clean_model(e, i)
        ids, rec = model_call(e.m, kind, p, P + 1, -1)
        assert ids.tolist() == full[: P + 1].tolist()
        if rec:
            assert_blank(rec, slice(0, P))
            assert_same_records(rec, full_rec, P + 1)
            assert rec[0][P] < 0 and (rec[1][P] >= 0).all()
        clean_model(e, i)


@pytest.mark.parametrize("kind", KINDS)
def test_batch_early_exits(env, kind):
    """2 sequences, the first leaves early and the second has room: each is what it is in the call without the exit"""
    e = env
    for pair in PAIRS:
        ps = [e.prompts[i] for i in pair]
        P0, P1 = len(ps[0]), len(ps[1])
        full, full_rec = batch_call(e.b2, kind, ps, TOTAL, -1)
        assert all(len(f) == TOTAL for f in full)
        # the first sequence's first id is the eos; the second runs until it meets that id, if it does
        eos = int(full[0][P0])
        ids, rec = batch_call(e.b2, kind, ps, TOTAL, eos)
        new1 = full[1][P1:].tolist()
        L1 = P1 + (new1.index(eos) if eos in new1 else len(new1))
        assert ids[0].tolist() == ps[0] and ids[1].tolist() == full[1][:L1].tolist()
        if rec:
            assert rec[0].shape == (2, TOTAL) and rec[1].shape == (2, TOTAL, N_TOP)
            assert_blank([r[0] for r in rec])
            assert_same_records([r[1] for r in rec], [r[1] for r in full_rec], L1)
            assert_blank([r[1] for r in rec], slice(L1, None))
        clean_batch(e, e.b2, ps, e.greedy_b2[pair])
        # no room after the first sequence's first id; the shorter prompt generates P0 + 1 - P1 ids
        ids, rec = batch_call(e.b2, kind, ps, P0 + 1, -1)
        assert ids[0].tolist() == full[0][: P0 + 1].tolist() and ids[1].tolist() == full[1][: P0 + 1].tolist()
        if rec:
            assert rec[0].shape == (2, P0 + 1)
            for q, Pq in ((0, P0), (1, P1)):
                assert_blank([r[q] for r in rec], slice(0, Pq))
                assert_same_records([r[q] for r in rec], [r[q] for r in full_rec], P0 + 1)
                assert (rec[0][q][Pq:] < 0).all()
        clean_batch(e, e.b2, ps, e.greedy_b2[pair])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_seq", [2, 16])
def test_serve_leaves_every_slot_clean(env, n_seq, kind):
    """5 prompts through 2 and 16 slots with per-prompt requests, tables and log-prob requests: afterwards no slot keeps any of it"""
    e = env
    b = e.b2 if n_seq == 2 else e.b16
    ks = [K, 0, K, K, 0]
    tables = [1, -1, 1, -1, 1]
    tops = [N_TOP, -1, 0, N_TOP, -1]
    if kind == "topk":
        ids, st = b.serve_topk(e.prompts, TOTAL, -1, ks, TEMP, SEED, slice_steps=4, max_new=MAX_NEW)
    elif kind == "biased":
        ids, st = b.serve_biased(e.prompts, TOTAL, -1, ks, TEMP, SEED, tables, None, slice_steps=4, max_new=MAX_NEW)
    else:
        ids, st, lp, ti, tl = b.serve_logprobs(e.prompts, TOTAL, -1, ks, TEMP, SEED, tops, tables, None, slice_steps=4, max_new=MAX_NEW)
        for j, p in enumerate(e.prompts):
            assert_blank((lp[j], ti[j], tl[j]), slice(0, len(p)))
            assert_blank((lp[j], ti[j], tl[j]), slice(len(ids[j]), None))
            if tops[j] < 0:
                assert_blank((lp[j], ti[j], tl[j]))
            else:
                assert (lp[j][len(p):len(ids[j])] < 0).all() and (ti[j][len(p):len(ids[j]), : tops[j]] >= 0).all() and (ti[j][:, tops[j]:] == -1).all()
    assert st["admissions"] == 5
    for j, p in enumerate(e.prompts):
        assert len(ids[j]) == len(p) + MAX_NEW and ids[j][: len(p)].tolist() == p
        if kind != "topk" and tables[j] >= 0:
            assert not set(ids[j][len(p):].tolist()) & set(e.banned)
        if ks[j] == 0 and (kind == "topk" or tables[j] < 0):
            assert ids[j].tolist() == e.serve_greedy[n_seq][j].tolist()
    if n_seq == 2:
        clean_batch(e, b, [e.prompts[1], e.prompts[0]], e.greedy_b2[(1, 0)])
    else:
        clean_batch(e, b, e.sixteen, e.greedy_b16)
    again, _ = b.serve(e.prompts, TOTAL, -1, 4, MAX_NEW)
    assert all(a.tolist() == g.tolist() for a, g in zip(again, e.serve_greedy[n_seq]))


@pytest.mark.parametrize("top_k", [K, 0])
def test_unused_extras_change_nothing(env, top_k):
    """no table, no log-prob request: top-k, biased and log-prob entry points agree id for id; top_k 0 is generate() / serve()"""
    e = env
    same = n = 0

    def count(ids, greedy):
        nonlocal same, n
        same, n = same + (ids.tolist() == greedy.tolist()), n + 1
    for i, p in enumerate(e.prompts):
        a = e.m.generate_topk(p, TOTAL, -1, top_k, TEMP, SEED, 5)
        b_ = e.m.generate_biased(p, TOTAL, -1, top_k, TEMP, SEED, 5)
        c = e.m.generate_logprobs(p, TOTAL, 0, -1, top_k, TEMP, SEED, 5)[0]      # (a model call always asks: 0 alternatives)
        assert a.tolist() == b_.tolist() == c.tolist(), i
        count(a, e.greedy_m[i])
    streams = [5, 6]
    for pair in PAIRS:
        ps = [e.prompts[i] for i in pair]
        a = e.b2.generate_topk(ps, TOTAL, -1, top_k, TEMP, SEED, streams)
        b_ = e.b2.generate_biased(ps, TOTAL, -1, top_k, TEMP, SEED, streams)
        c = e.b2.generate_logprobs(ps, TOTAL, None, -1, top_k, TEMP, SEED, streams)[0]
        for q in range(2):
            assert a[q].tolist() == b_[q].tolist() == c[q].tolist(), (pair, q)
            count(a[q], e.greedy_b2[pair][q])
    for n_seq, b in ((2, e.b2), (16, e.b16)):
        a, _ = b.serve_topk(e.prompts, TOTAL, -1, top_k, TEMP, SEED, slice_steps=4, max_new=MAX_NEW)
        b_, _ = b.serve_biased(e.prompts, TOTAL, -1, top_k, TEMP, SEED, slice_steps=4, max_new=MAX_NEW)
        c = b.serve_logprobs(e.prompts, TOTAL, -1, top_k, TEMP, SEED, None, slice_steps=4, max_new=MAX_NEW)[0]
        for j in range(5):
            assert a[j].tolist() == b_[j].tolist() == c[j].tolist(), (n_seq, j)
            count(a[j], e.serve_greedy[n_seq][j])
    assert same == n if top_k == 0 else same < n          # (sampled: something differs from greedy, or the request never arrived)
