"""-m gpu: what the four host generation modes (greedy, top-k, bias tables, log-prob records) share above the C ABI -- the exits
that leave a call early, the state a call leaves behind, and the extras a call does not use.

Each mode sets up to three things on a decoder slot (sampling request, table binding, log-prob request) and has to take back
exactly those on every way out.  Held here, on a HostModel, a HostBatch of 2 and serve on 2 and 16 slots:
  * a call whose first id is the eos, or that has no room after the first id, returns the prompt (plus that id) with blank records;
  * after every call no sequence is bound, plain generate() gives the greedy ids it gave before anything was set, and a step
    the caller drives writes no record;
  * with no table and no log-prob request the three sampled entry points and the three sampled serves return the same ids, and
    with top_k 0 those are generate()'s and serve()'s.

The nucleus, penalized, fsm and mirostat forms are held to the same: with every upper feature off each of the seven sampled forms
returns the top-k form's ids -- the one form that cannot name an upper stage -- and leaves the decoder's cut, penalty, automaton and
Mirostat state as it found it, "ever used" flags included."""
import numpy as np
import pytest

import bias_ref as bref
import fsm_ref
from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from test_bias_gpu import model_setup, upload
from test_fsm_gpu import SEED as FSM_SEED      # (the seed test_fsm_gpu.existing draws with)
from test_fsm_gpu import existing

pytestmark = pytest.mark.gpu

NINF = -np.inf
LENGTHS = [3, 5, 17, 20, 40]          # below and at or above 16: at 16 slots serve takes both prompt paths
TOTAL, MAX_NEW = 52, 10
K, TEMP, SEED = 40, 0.9, 77
N_TOP = 3
PAIRS = [(1, 0), (3, 2), (4, 3)]      # (longer, shorter) prompts of a 2-sequence batch: the longer one gets the early exit
KINDS = ["topk", "biased", "logprobs", "nucleus", "penalized", "fsm", "mirostat"]


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
    if kind == "fsm":            # (an automaton and a table do not compose: this form carries records only)
        ids, _, lp, ti, tl = m.generate_fsm(prompt, total, -1, eos, K, TEMP, SEED, 5, n_top=N_TOP)
        return ids, (lp, ti, tl)
    if kind == "mirostat":       # (tau 0: off; the binding passes no record outputs)
        return m.generate_mirostat(prompt, total, 0.0, 0.1, eos, K, TEMP, SEED, 5, table=1), None
    call = {"logprobs": m.generate_logprobs, "nucleus": m.generate_nucleus, "penalized": m.generate_penalized}[kind]
    ids, lp, ti, tl = call(prompt, total, eos=eos, top_k=K, temp=TEMP, seed=SEED, stream=5, table=1, n_top=N_TOP)
    return ids, (lp, ti, tl)


def batch_call(b, kind, prompts, total, eos):
    """(ids per sequence, records [n_seq][total] or None) of one fixed-batch call of `kind`"""
    streams = [5, 6]
    if kind == "topk":
        return b.generate_topk(prompts, total, eos, K, TEMP, SEED, streams), None
    if kind == "biased":
        return b.generate_biased(prompts, total, eos, K, TEMP, SEED, streams, [1, 1], None), None
    if kind == "fsm":            # (the binding passes no record outputs through this form's fixed batch)
        return b.generate_fsm(prompts, total, -1, eos, K, TEMP, SEED, streams, tables=[1, 1])[0], None
    if kind == "mirostat":
        return b.generate_mirostat(prompts, total, 0.0, 0.1, eos, K, TEMP, SEED, streams, tables=[1, 1]), None
    call = {"logprobs": b.generate_logprobs, "nucleus": b.generate_nucleus, "penalized": b.generate_penalized}[kind]
    ids, lp, ti, tl = call(prompts, total, eos=eos, top_k=K, temp=TEMP, seed=SEED, streams=streams, tables=[1, 1], n_top=N_TOP)
    return ids, (lp, ti, tl)


def lists(ids):
    return ids.tolist() if isinstance(ids, np.ndarray) else [a.tolist() for a in ids]


def stages(o):
    """the "ever used" flags of a decoder's cut, penalty, automaton and Mirostat stages -- and nobody is bound to any of them"""
    cut, pen, fsm, miro = o.cut_info(), o.penalty_info(), o.fsm_info(), o.mirostat_info()
    assert np.all(np.asarray(cut[0]) == 1.0) and np.all(np.asarray(cut[1]) == 0.0)
    assert np.all(np.asarray(pen[0]) == 1.0) and np.all(np.asarray(pen[1]) == 0.0) and np.all(np.asarray(pen[2]) == 0.0)
    assert np.all(np.asarray(fsm[1]) == -1) and not np.asarray(miro[0]).any()
    return cut[3], pen[5], fsm[3], miro[3]


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
        if kind not in ("topk", "fsm"):                   # (the two single-sequence forms that run without table 1)
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
    elif kind == "mirostat":
        ids, st = b.serve_mirostat(e.prompts, TOTAL, -1, ks, TEMP, SEED, 0.0, 0.1, tables=tables, slice_steps=4, max_new=MAX_NEW)
    else:
        if kind == "logprobs":
            ids, st, lp, ti, tl = b.serve_logprobs(e.prompts, TOTAL, -1, ks, TEMP, SEED, tops, tables, None, slice_steps=4, max_new=MAX_NEW)
        elif kind == "fsm":
            ids, st, _, lp, ti, tl = b.serve_fsm(e.prompts, TOTAL, -1, ks, TEMP, SEED, -1, tables=tables, n_top=tops, slice_steps=4, max_new=MAX_NEW)
        else:
            call = b.serve_nucleus if kind == "nucleus" else b.serve_penalized
            ids, st, lp, ti, tl = call(e.prompts, TOTAL, -1, ks, TEMP, SEED, tables=tables, n_top=tops, slice_steps=4, max_new=MAX_NEW)
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


def model_forms(m, p, top_k):
    """prompt p through the seven sampled single-sequence forms, every upper feature off: (name, ids), top-k first"""
    yield "topk", m.generate_topk(p, TOTAL, -1, top_k, TEMP, SEED, 5)
    yield "biased", m.generate_biased(p, TOTAL, -1, top_k, TEMP, SEED, 5)
    yield "logprobs", m.generate_logprobs(p, TOTAL, 0, -1, top_k, TEMP, SEED, 5)[0]      # (this form always asks: 0 alternatives)
    yield "nucleus", m.generate_nucleus(p, TOTAL, -1, top_k, TEMP, SEED, 5)
    yield "penalized", m.generate_penalized(p, TOTAL, -1, top_k, TEMP, SEED, 5)
    yield "fsm", m.generate_fsm(p, TOTAL, -1, -1, top_k, TEMP, SEED, 5)[0]
    yield "mirostat", m.generate_mirostat(p, TOTAL, 0.0, 0.1, -1, top_k, TEMP, SEED, 5)


def batch_forms(b, ps, top_k, streams):
    yield "topk", b.generate_topk(ps, TOTAL, -1, top_k, TEMP, SEED, streams)
    yield "biased", b.generate_biased(ps, TOTAL, -1, top_k, TEMP, SEED, streams)
    yield "logprobs", b.generate_logprobs(ps, TOTAL, None, -1, top_k, TEMP, SEED, streams)[0]
    yield "nucleus", b.generate_nucleus(ps, TOTAL, -1, top_k, TEMP, SEED, streams)
    yield "penalized", b.generate_penalized(ps, TOTAL, -1, top_k, TEMP, SEED, streams)
    yield "fsm", b.generate_fsm(ps, TOTAL, -1, -1, top_k, TEMP, SEED, streams)[0]
    yield "mirostat", b.generate_mirostat(ps, TOTAL, 0.0, 0.1, -1, top_k, TEMP, SEED, streams)


def serve_forms(b, ps, top_k):
    kw = dict(slice_steps=4, max_new=MAX_NEW)
    yield "topk", b.serve_topk(ps, TOTAL, -1, top_k, TEMP, SEED, **kw)[0]
    yield "biased", b.serve_biased(ps, TOTAL, -1, top_k, TEMP, SEED, **kw)[0]
    yield "logprobs", b.serve_logprobs(ps, TOTAL, -1, top_k, TEMP, SEED, None, **kw)[0]
    yield "nucleus", b.serve_nucleus(ps, TOTAL, -1, top_k, TEMP, SEED, **kw)[0]
    yield "penalized", b.serve_penalized(ps, TOTAL, -1, top_k, TEMP, SEED, **kw)[0]
    yield "fsm", b.serve_fsm(ps, TOTAL, -1, top_k, TEMP, SEED, -1, **kw)[0]
    yield "mirostat", b.serve_mirostat(ps, TOTAL, -1, top_k, TEMP, SEED, 0.0, 0.1, **kw)[0]


@pytest.mark.parametrize("top_k", [K, 0])
def test_unused_extras_change_nothing(env, top_k):
    """no table, no log-prob request, cut (1, 0), penalty (1, 0, 0), no automaton, tau 0: each of the seven sampled forms returns the
    top-k form's ids, id for id, on a model, a batch of 2 and through serve at 2 and 16 slots; top_k 0 is generate() / serve().  After
    every call the cut, the penalty, the automaton and Mirostat report nobody bound and their "ever used" flags are as before it."""
    e = env
    same = n = 0

    def count(ids, greedy):
        nonlocal same, n
        same, n = same + (ids.tolist() == greedy.tolist()), n + 1

    def agree(o, forms, where, greedy, want):
        """every form's ids are the first form's (top-k's); after each call the decoder's upper stages are as they were and the plain
        greedy call `greedy` gives the ids `want` recorded in the fixture"""
        before, first = stages(o), None
        for name, ids in forms:                            # (a generator: this body runs right after the form's call)
            assert stages(o) == before, (where, name)
            assert lists(greedy()) == lists(want), (where, name)
            first = ids if first is None else first
            assert lists(ids) == lists(first), (where, name)
        return first
    for i, p in enumerate(e.prompts):
        count(agree(e.m, model_forms(e.m, p, top_k), i, lambda: e.m.generate(p, TOTAL), e.greedy_m[i]), e.greedy_m[i])
    for pair in PAIRS:
        ps = [e.prompts[i] for i in pair]
        a = agree(e.b2, batch_forms(e.b2, ps, top_k, [5, 6]), pair, lambda: e.b2.generate(ps, TOTAL), e.greedy_b2[pair])
        for q in range(2):
            count(a[q], e.greedy_b2[pair][q])
    for n_seq, b in ((2, e.b2), (16, e.b16)):
        a = agree(b, serve_forms(b, e.prompts, top_k), n_seq, lambda: b.serve(e.prompts, TOTAL, -1, 4, MAX_NEW)[0], e.serve_greedy[n_seq])
        for j in range(5):
            count(a[j], e.serve_greedy[n_seq][j])
    assert same == n if top_k == 0 else same < n          # (sampled: something differs from greedy, or the request never arrived)


# ---- one request that uses every stage that composes, through the _mirostat forms (the only ones that can pass them all): item A is
# a table (with min_new) + records + a penalty + Mirostat, item B an automaton + a penalty + a cut.  The reference is put together from
# what the per-feature tests use: the first id by the row operators on the prompt's logits (gten_hip_sample_rows_miro for A; for B
# tests/test_fsm_gpu.py's `existing` -- the penalised cut operator under the bias row that restates the state's mask), every later id
# by the decoder driven step by step from here with the requests set through the set_* calls, teacher-forced with the ids under test.
# (The queue is not held to this reference here: serve_mirostat with these two items among the five prompts, slices of 4 steps, gives
# item A another id at position P + 8 than the single call does -- 377 where this reference has 149 -- and gave the same before the
# levels were collapsed; host/serve.h's scheduler is outside this test's subject.)
A = dict(j=1, stream=1, tau=3.0, eta=0.25, rep=1.3, freq=0.1, pres=0.0, last_n=0, min_new=6, n_top=N_TOP)
B = dict(j=3, stream=3, state=2, rep=1.2, freq=0.0, pres=0.2, last_n=8, top_p=0.9, min_p=0.02)
TAU_Q = 3 << 16                       # tau 3.0 in Q16; the first id is drawn from mu = 2 tau


def raw_model_mirostat(e, p, stream, table=-1, min_new=0, n_top=-1, top_p=1.0, min_p=0.0, rep=1.0, freq=0.0, pres=0.0, last_n=0, state=-1, tau=0.0,
                       eta=0.1):
    """gten_host_model_generate_mirostat with record outputs (the Python wrapper passes none): (ids, (lp, top ids, top lps) or None)"""
    import ctypes as C
    H = load_package().hostabi
    ask, w = n_top >= 0, max(n_top, 0)
    buf = np.zeros(TOTAL, np.int32)
    buf[: len(p)] = p
    lp, ti, tl = np.zeros(TOTAL, np.float32), np.full((TOTAL, w), -1, np.int32), np.zeros((TOTAL, w), np.float32)
    pen, ended = H._penalty_arg(1, float(rep), float(freq), float(pres), int(last_n), True), np.zeros(1, np.int32)
    total = e.host._generate_miro(e.m.h, H._ptr(buf), len(p), TOTAL, -1, K, TEMP, C.c_uint64(FSM_SEED), C.c_uint32(stream), table, min_new, n_top,
                                  C.c_float(top_p), C.c_float(min_p), H._ptr(lp) if ask else None, H._ptr(ti) if ask else None,
                                  H._ptr(tl) if ask else None, C.byref(pen), state, H._ptr(ended), C.c_float(tau), C.c_float(eta))
    assert total == TOTAL and ended[0] == 0
    return buf, ((lp, ti, tl) if ask else None)


def raw_batch_mirostat(e, ps):
    """gten_host_batch_generate_mirostat on (A's prompt, B's prompt) with record outputs: (ids per sequence, (lp, top ids, top lps))"""
    import ctypes as C
    H = load_package().hostabi
    args, rec = H._records([A["n_top"], -1], 2, TOTAL)
    pen = H._penalty_arg(2, [A["rep"], B["rep"]], [A["freq"], B["freq"]], [A["pres"], B["pres"]], [A["last_n"], B["last_n"]], True)
    st, ended = np.array([-1, B["state"]], np.int32), np.zeros(2, np.int32)
    ta, et = np.array([A["tau"], 0.0], np.float32), np.array([A["eta"], 0.1], np.float32)
    ids = e.b2._generate(e.host._bgen_miro, "batch_generate_mirostat", ps, TOTAL, -1,
                         H._request_args(2, K, TEMP, FSM_SEED) + H._full_args(2, ([A["stream"], B["stream"]], np.uint32), ([1, -1], np.int32),
                                                                            ([A["min_new"], 0], np.int32)),
                         args + H._cut_args(2, [1.0, B["top_p"]], [0.0, B["min_p"]]) + [C.byref(pen), H._ptr(st), H._ptr(ended), H._ptr(ta), H._ptr(et),
                                                                                       C.c_float(0.0), C.c_float(0.1)])
    assert not ended.any()
    return ids, rec


def driven_by_hand(m, got, P):
    """the ids the model's decoder commits at positions (P, len(got)) when every step is driven from here, teacher-forced with `got`
    (the prompt's rows are in the caches: the caller has just read its logits)"""
    m.decode_begin(got)
    out = []
    for n in range(P + 1, len(got)):
        m.decode_step(n, use_graph=n % 2 == 0)
        out.append(m.decode_result(n))
    return out


def test_a_composed_request_through_the_mirostat_forms(env, hip):
    e, m, V = env, env.m, env.cfg.n_vocab
    pkg = load_package()
    f = pkg.hostabi.Fsm(e.host, V)
    f.add_table(*fsm_ref.random_pool(np.random.default_rng(31), 16, V, 0.25, 0))          # sixteen live states, a quarter of the ids each
    nxt, flags = f.tables()
    for o in (m, e.b2, e.b16):
        o.set_fsm(f)
    table = bref.table(V, [(j, NINF) for j in e.banned])
    pa, pb = e.prompts[A["j"]], e.prompts[B["j"]]
    Pa, Pb = len(pa), len(pb)
    # -- item A alone on the model
    ga, rec = raw_model_mirostat(e, pa, A["stream"], table=1, min_new=A["min_new"], n_top=A["n_top"], rep=A["rep"], freq=A["freq"], pres=A["pres"],
                                 last_n=A["last_n"], tau=A["tau"], eta=A["eta"])
    assert ga[:Pa].tolist() == pa and not set(ga[Pa:Pa + A["min_new"]].tolist()) & set(e.banned)
    row = upload(hip, m.logits(pa, 0))[0]
    ids, _, info = hip.sample_rows_miro(row, 1, V, V, K, TEMP, FSM_SEED, A["stream"], Pa, 2 * TAU_Q, A["tau"], A["eta"], bias=upload(hip, table)[0],
                                        bias_stride=0, hist=[np.asarray(pa, np.int32)], r=A["rep"], freq=A["freq"], pres=A["pres"])
    assert int(ids[0]) == int(ga[Pa])
    first_rec = hip.row_top_logprobs(row, 1, V, V, int(ids[0]), A["n_top"])
    m.set_sampling(K, TEMP, FSM_SEED, A["stream"])
    assert m.set_seq_bias_rc(1, Pa + A["min_new"]) == 0
    m.set_logprobs(A["n_top"])
    m.set_penalty(A["rep"], A["freq"], A["pres"], 0, A["last_n"])
    m.set_mirostat(A["tau"], A["eta"], int(info[0]["mu_next"]), Pa + 1)
    assert driven_by_hand(m, ga, Pa) == ga[Pa + 1:].tolist()
    want = m.logprobs(Pa + 1, TOTAL - Pa - 1, A["n_top"])
    m.set_mirostat(0.0, 0.1, 0, 0)
    m.set_penalty()
    m.set_logprobs(-1)
    assert m.set_seq_bias_rc(-1) == 0
    m.set_sampling(0)
    assert_blank(rec, slice(0, Pa))
    assert_same_records([r[Pa:Pa + 1] for r in rec], [first_rec[0], first_rec[1], first_rec[2]], 1)
    assert_same_records([r[Pa + 1:] for r in rec], want, TOTAL - Pa - 1)
    # -- item B alone on the model
    gb, _ = raw_model_mirostat(e, pb, B["stream"], top_p=B["top_p"], min_p=B["min_p"], rep=B["rep"], freq=B["freq"], pres=B["pres"], last_n=B["last_n"],
                               state=B["state"])
    hist = np.asarray(pb[Pb - B["last_n"]:], np.int32)
    ids, _ = existing(hip, m.logits(pb, 0)[None], fsm_ref.bias_of(nxt, flags, B["state"], V)[None], K, TEMP, B["stream"], Pb, B["top_p"], B["min_p"],
                      ([hist], B["rep"], B["freq"], B["pres"]))
    assert int(ids[0]) == int(gb[Pb]) and nxt[B["state"]][gb[Pb]] != fsm_ref.DEAD
    m.set_sampling(K, TEMP, FSM_SEED, B["stream"])
    m.set_cut(B["top_p"], B["min_p"])
    m.set_penalty(B["rep"], B["freq"], B["pres"], 0, B["last_n"])
    m.set_seq_fsm(int(nxt[B["state"]][gb[Pb]]), Pb + 1)
    assert driven_by_hand(m, gb, Pb) == gb[Pb + 1:].tolist()
    m.set_seq_fsm(-1, 0)
    m.set_penalty()
    m.set_cut()
    m.set_sampling(0)
    state = B["state"]
    for t in gb[Pb:]:                                                                      # every new id walks the automaton
        state = int(nxt[state][t])
        assert state != fsm_ref.DEAD
    assert m.generate_topk(pb, TOTAL, -1, K, TEMP, FSM_SEED, B["stream"]).tolist() != gb.tolist()
    # -- both as one batch of 2, with A's records
    ids, brec = raw_batch_mirostat(e, [pa, pb])
    assert ids[0].tolist() == ga.tolist() and ids[1].tolist() == gb.tolist()
    assert_same_records([r[0] for r in brec], rec, TOTAL)
    assert_blank([r[1] for r in brec])
    # -- nothing is left behind on any decoder
    for o in (m, e.b2, e.b16):
        stages(o)
        o.set_fsm(None)
    clean_model(e, 0)
    clean_batch(e, e.b2, [e.prompts[1], e.prompts[0]], e.greedy_b2[(1, 0)])
    f.close()
