"""-m gpu: Mirostat v2 in the decoder (include/gten_hip_mirostat.h, include/gten_host_mirostat.h).

k_dec_sample_miro is held to the row operator (which tests/test_mirostat_gpu.py holds to the restatement): on every step's own logits,
with the mu the sequence's row holds at that position, the step's id and the mu it commits are the operator's, bit for bit -- through
captured single steps, eager steps and four-step graph replays, beside greedy, unbound, cut, penalised, table-bound and automaton-bound
sequences in one decoder.  Sequences without Mirostat give the ids and record bytes of the run in which nobody was bound."""
import numpy as np
import pytest

import bias_ref as bref
import fsm_ref
import miro_ref as ref
from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from test_bias_gpu import NINF, SEED, TOTAL, Dec, P, upload
from test_fsm_gpu import dec_bind, dec_states, weights_into
from test_logprobs_gpu import bits, dec_ask, dec_records
from test_nucleus_gpu import dec_cut, model_setup
from test_penalty_gpu import dec_pen
from test_sampler_levels_gpu import PATTERN

pytestmark = pytest.mark.gpu

TAU, ETA = 4.0, 0.25
TAU_Q, ETA_Q = 4 << 16, 16384
PEN = (1.3, 0.2, 0.1)
CUT = (0.8, 0.1)
TABLE = 1
N_KINDS = 7


def dec_miro(d, q, tau, eta=ETA, mu=None, pos=0):
    d.o.set_mirostat(tau, eta, mu, pos) if d.one else d.o.set_mirostat(q, tau, eta, mu, pos)


def dec_miro_rc(d, q, tau, eta=ETA, mu=None, pos=0):
    return d.o.set_mirostat_rc(tau, eta, mu, pos) if d.one else d.o.set_mirostat_rc(q, tau, eta, mu, pos)


def dec_mus(d, q, n_from, count):
    return d.o.mirostat_mus(n_from, count) if d.one else d.o.mirostat_mus(q, n_from, count)


def mixed(n_seq, shift, V):
    """per sequence, by kind = (q + shift) % 7: 0 greedy and bound (Mirostat is ignored, the mu row not touched); 1 top-k 40; 2 top-k 40, bound;
    3 the whole vocabulary, bound, penalised; 4 top-k 40, bound, under a -inf table; 5 the whole vocabulary under a cut, not bound;
    6 top-k 40, bound, in a state of an automaton that masks every step.  n_top cycles through -1 / 0 / 3."""
    kinds = [(q + shift) % N_KINDS for q in range(n_seq)]
    ks = np.array([0 if kd == 0 else V if kd in (3, 5) else 40 for kd in kinds], np.int32)
    tops = np.array([(-1, 0, 3)[((q + shift) // 2) % 3] for q in range(n_seq)], np.int32)
    return kinds, ks, tops


def request_all(d, kinds, ks, tops, streams, on):
    """every sequence's requests (on False: cleared); the Mirostat bindings are set apart"""
    for q, kd in enumerate(kinds):
        d.request(q, int(ks[q]) if on else 0, 0.9, SEED, int(streams[q]))
        dec_ask(d, q, int(tops[q]) if on else -1)
        if kd == 3:
            dec_pen(d, q, *(PEN if on else (1.0, 0.0, 0.0)))
        if kd == 4:
            assert d.bind_rc(q, TABLE if on else -1) == 0
        if kd == 5:
            dec_cut(d, q, *(CUT if on else (1.0, 0.0)))
        if kd == 6:
            dec_bind(d, q, (5 * q + 2) % 12 if on else -1, P + 1)


def bind_all(d, kinds, on, mu0):
    for q, kd in enumerate(kinds):
        if kd in (0, 2, 3, 4, 6):
            dec_miro(d, q, TAU if on else 0.0, ETA, int(mu0[q]), P + 1)


def run(d, prompts, tf, pattern, want_logits=False):
    """teacher-forced with tf, every position by `pattern`; returns ids [n_seq][positions] and, for an all-single-step pattern, the
    logits of every step [positions][n_seq][V]"""
    for q in range(d.n):
        d.prefill(q, prompts[q])
        d.begin(q, tf[q])
    n, logits = P + 1, []
    for kind in pattern:
        if kind == "steps4":
            d.o.decode_steps(n, 4)
        else:
            d.o.decode_step(n, use_graph=(kind == "graph"))
            if want_logits:
                logits.append(np.stack([d.logits(q) for q in range(d.n)]))
        n += 4 if kind == "steps4" else 1
    assert n == TOTAL
    return np.array([[d.result(q, m) for m in range(P + 1, TOTAL)] for q in range(d.n)]), logits


def operator_step(hip, pool, nxt, row, V, kd, k, stream, n, mu, hist, table, state):
    """(id, mu_next) of one sequence's step by gten_hip_sample_rows_miro on the step's own logits"""
    kw = {}
    if kd == 3:
        kw.update(hist=[hist], r=PEN[0], freq=PEN[1], pres=PEN[2])
    if kd == 4:
        kw.update(bias=upload(hip, table)[0], bias_stride=0)
    if kd == 6:
        kw.update(pool=pool, states=[state])
    ids, after, info = hip.sample_rows_miro(upload(hip, row)[0], 1, V, V, k, 0.9, SEED, stream, n, mu, TAU, ETA, **kw)
    return int(ids[0]), int(info[0]["mu_next"]), int(info[0]["n_keep"]), int(info[0]["n_cand"])


@pytest.mark.parametrize("n_seq,n_vocab", [(1, 512), (2, 512), (16, 512), (128, 512), (1, 2048), (2, 2048), (16, 2048)])
def test_decoder_follows_the_operator_on_its_own_logits(hip, n_seq, n_vocab):
    """n_vocab 512: every bound sequence runs on compacted candidates; 2048: the whole-vocabulary kinds run the row-wide routine"""
    pkg = load_package()
    host = pkg.load_host()
    cfg, weights = model_setup(host, n_vocab)
    V = cfg.n_vocab
    d = Dec(host, cfg, weights, n_seq)
    prompts = [list(host.synthetic_tokens(P, seed=700 + q, n_vocab=V)) for q in range(n_seq)]
    tf = [d.o.generate(prompts[0], TOTAL)] if d.one else d.o.generate(prompts, TOTAL)            # the ids every run is teacher-forced with
    streams = np.arange(n_seq, dtype=np.uint32) * 3 + 1
    banned = sorted({int(g[p]) for g in tf for p in (P, P + 1, P + 2)})[: V // 2]
    d.o.set_bias_table(TABLE, [(j, NINF) for j in banned])
    table = bref.table(V, [(j, NINF) for j in banned])
    f = pkg.hostabi.Fsm(host, V)
    f.add_table(*fsm_ref.random_pool(np.random.default_rng(31), 12, V, 0.25, 0))                # twelve live states, a quarter of the ids each
    nxt, flags = f.tables()
    d.o.set_fsm(f)
    pool = hip.fsm_upload(nxt, flags)
    singles = ["graph" if i % 2 == 0 else "eager" for i in range(TOTAL - P - 1)]
    shifts = range(N_KINDS) if n_seq == 1 else (0, 2, 4, 6) if n_seq == 2 else (0,)
    check = list(range(n_seq))                                                                   # every sequence's every step is held to the operator
    assert not d.o.mirostat_info()[3] and (dec_mus(d, 0, 0, 4) == 0).all()
    cut_proper = moved = 0
    for shift in shifts:
        kinds, ks, tops = mixed(n_seq, shift, V)
        mu0 = np.array([(1 << 16, 3 << 16, 2 * TAU_Q)[q % 3] for q in range(n_seq)], np.int64)
        bound = [q for q in range(n_seq) if kinds[q] in (0, 2, 3, 4, 6)]
        # nobody bound: on the first shift the decoder has never heard of Mirostat and launches what it always did
        request_all(d, kinds, ks, tops, streams, True)
        base, logits = run(d, prompts, tf, singles, want_logits=True)
        base_rec = {q: dec_records(d, q, P + 1, TOTAL - P - 1, int(tops[q])) for q in range(n_seq) if tops[q] >= 0}
        assert d.o.mirostat_info()[3] == (shift != shifts[0])
        # bound: captured steps, eager steps and four-step replays
        bind_all(d, kinds, True, mu0)
        tq, eq, ps, on = d.o.mirostat_info()
        assert on and [int(tq[q]) for q in bound] == [TAU_Q] * len(bound) and [int(eq[q]) for q in bound] == [ETA_Q] * len(bound)
        assert all(ps[q] == P + 1 for q in bound) and not any(tq[q] for q in range(n_seq) if q not in bound)
        before = {q: dec_mus(d, q, P + 1, TOTAL - P) for q in bound}
        got, _ = run(d, prompts, tf, PATTERN)
        mus = {q: dec_mus(d, q, P + 1, TOTAL - P) for q in bound}
        rec = {q: dec_records(d, q, P + 1, TOTAL - P - 1, int(tops[q])) for q in range(n_seq) if tops[q] >= 0}
        for q in range(n_seq):
            if kinds[q] in (0, 1, 5):
                # without Mirostat (or greedy): the ids and record bytes of the run in which nobody was bound
                assert got[q].tolist() == base[q].tolist(), (shift, q, kinds[q])
                if tops[q] >= 0:
                    for a, b in zip(rec[q], base_rec[q]):
                        assert (bits(a) == bits(b)).all() if a.dtype == np.float32 else a.tolist() == b.tolist(), (shift, q)
            else:
                moved += got[q].tolist() != base[q].tolist()
            if kinds[q] == 0:
                assert mus[q][0] == mu0[q] and mus[q].tolist() == before[q].tolist(), (shift, q)  # a greedy sequence leaves its mu row alone
            if kinds[q] == 4:
                assert all(table[j] > NINF for j in got[q]), (shift, q)
        # every checked step against the operator on that step's logits, with the mu the row holds there
        for q in check:
            kd = kinds[q]
            if kd not in (2, 3, 4, 6):
                continue
            assert int(mus[q][0]) == mu0[q]
            states = dec_states(d, q, P + 1, TOTAL - P) if kd == 6 else None
            for i, n in enumerate(range(P + 1, TOTAL)):
                id_, mu_next, n_keep, n_cand = operator_step(hip, pool, nxt, logits[i][q], V, kd, int(ks[q]), int(streams[q]), n, int(mus[q][i]),
                                                             [int(t) for t in tf[q][:n]], table, int(states[i]) if kd == 6 else -1)
                assert (id_, mu_next) == (int(got[q][i]), int(mus[q][i + 1])), (shift, q, kd, n)
                cut_proper += 1 < n_keep < n_cand
                if tops[q] >= 0:
                    # the record: from the raw row and the committed id, whatever the id was drawn under
                    olp, oti, otl = hip.row_top_logprobs(upload(hip, logits[i][q])[0], 1, V, V, id_, int(tops[q]))
                    assert bits(rec[q][0][i]) == bits(olp[0]) and rec[q][1][i][: tops[q]].tolist() == oti[0].tolist(), (shift, q, n)
            assert int(dec_mus(d, q, TOTAL + 1, 1)[0]) == 0                                      # nothing behind the last commit was written
        # step by step, with two steps repeated: the same ids, the same mu row (a repeat reads mu[n], rewrites mu[n + 1])
        for q in range(n_seq):
            d.prefill(q, prompts[q])
            d.begin(q, tf[q])
        for i, n in enumerate(range(P + 1, TOTAL)):
            for rep in range(2 if n in (P + 3, TOTAL - 1) else 1):
                d.o.decode_step(n, use_graph=(n + rep) % 2 == 0)
                assert [d.result(q, n) for q in range(n_seq)] == got[:, i].tolist(), (shift, n, rep)
        for q in bound:
            assert dec_mus(d, q, P + 1, TOTAL - P).tolist() == mus[q].tolist(), (shift, q)
        # a binding at a later position ignores what the earlier run left in the row; the step before it draws without Mirostat
        q0 = next((q for q in check if kinds[q] == 2), None)
        if q0 is not None:
            n0, other = P + 9, 11 << 16
            assert int(mus[q0][n0 - P - 1]) != other
            dec_miro(d, q0, TAU, ETA, other, n0)
            assert int(dec_mus(d, q0, n0, 1)[0]) == other
            d.o.decode_step(n0, use_graph=True)
            id_, mu_next, _, _ = operator_step(hip, pool, nxt, d.logits(q0), V, 2, 40, int(streams[q0]), n0, other, [], table, -1)
            assert d.result(q0, n0) == id_ and dec_mus(d, q0, n0, 2).tolist() == [other, mu_next]
            d.o.decode_step(n0 - 1, use_graph=False)
            free = hip.sample_rows(upload(hip, d.logits(q0))[0], 1, V, V, 40, 0.9, SEED, int(streams[q0]), n0 - 1)
            assert d.result(q0, n0 - 1) == int(free[0]) and int(dec_mus(d, q0, n0, 1)[0]) == other
        # unbinding restores the ids of the run in which nobody was bound
        bind_all(d, kinds, False, mu0)
        assert not d.o.mirostat_info()[0].any() and d.o.mirostat_info()[3]
        again, _ = run(d, prompts, tf, PATTERN)
        assert again.tolist() == base.tolist(), shift
        request_all(d, kinds, ks, tops, streams, False)
        assert d.sampler_launches() == 0                                                         # no sampler launch once everything is cleared
    assert cut_proper >= 1 and moved >= 1                                                        # (the threshold cut something somewhere, and ids moved)
    f.close()
    d.o.close()


def test_a_slot_that_repeats_its_last_step_leaves_the_same_mu(hip):
    """gten_hip_decoder_slot_start_until inside a free-running run of 32 shared steps: slot 0 reaches its last step after 11 steps and
    repeats it 21 times while slot 1 runs on.  Every repeat reads the same mu[last] and rewrites the same mu[last + 1]: the mu row is
    that of the same slot running on without a last step, and the entry behind it is untouched"""
    host = load_package().load_host()
    cfg, weights = model_setup(host, 512)
    V = cfg.n_vocab
    b = weights_into(host.batch(cfg, 2), weights)
    prompts = [list(host.synthetic_tokens(P, seed=620 + q, n_vocab=V)) for q in range(2)]
    streams = np.array([4, 9], np.uint32)
    rows = np.stack([b.prefill(q, prompts[q]) for q in range(2)])
    # the prompt's first id by the operator, the decoder bound at the next position with the mu_next it returns
    id0, _, info0 = hip.sample_rows_miro(upload(hip, rows)[0], 2, V, V, 40, 0.9, SEED, streams, P, 2 * TAU_Q, TAU, ETA)
    dec = b.fsm_decoder()
    last0, steps = P + 11, 32

    def run_until(last):
        for q in range(2):
            b.decode_begin(q, prompts[q] + [int(id0[q])])
            b.set_sampling(q, 40, 0.9, SEED, int(streams[q]))
            b.set_mirostat(q, TAU, ETA, int(info0[q]["mu_next"]), P + 1)
        hip.decoder_slot_start_until(dec, 0, P + 1, last)
        hip.decoder_slot_start_until(dec, 1, P + 1, 0)
        hip.decoder_run(dec, steps)
        n0 = (last or P + steps) - P
        return hip.decoder_slot_ids(dec, 0, P + 1, n0), hip.decoder_slot_ids(dec, 1, P + 1, steps)

    free0, free1 = run_until(0)                                                                  # no last step: both run on
    mu_free = [b.mirostat_mus(q, P + 1, steps + 1) for q in range(2)]
    assert len(set(mu_free[0].tolist())) > 8 and int(b.mirostat_mus(0, P + steps + 2, 1)[0]) == 0
    b.set_mirostat(0, TAU, ETA, 12345, last0 + 2)                                                # (a mark behind the last commit of the run below)
    ids0, ids1 = run_until(last0)
    assert len(ids0) == 11 and ids0.tolist() == free0[:11].tolist() and ids1.tolist() == free1.tolist()
    assert b.mirostat_mus(0, P + 1, 12).tolist() == mu_free[0][:12].tolist()                     # mu[last + 1] is the one commit's, 21 times over
    assert b.mirostat_mus(1, P + 1, steps + 1).tolist() == mu_free[1].tolist()
    assert b.mirostat_mus(0, last0 + 2, 4).tolist() == [12345] + mu_free[0][13:16].tolist()      # ... and nothing behind it was written
    # (the raw handle's readers and setter: the same rows, the same bindings)
    assert hip.decoder_slot_mus(dec, 1, P + 1, 5).tolist() == mu_free[1][:5].tolist()
    tq, eq, ps, on, row = hip.decoder_mirostat_info(dec, 2, row_seq=1, row_from=P + 1, row_count=3)
    assert on and tq.tolist() == [TAU_Q] * 2 and eq.tolist() == [ETA_Q] * 2 and ps.tolist() == [P + 1] * 2 and row.tolist() == mu_free[1][:3].tolist()
    for q in range(2):
        hip.decoder_slot_park(dec, q)
        hip.decoder_set_seq_mirostat(dec, q, 0.0)
        b.set_sampling(q, 0)
    assert not b.mirostat_info()[0].any()
    b.close()


def test_requests_are_checked_and_read_back(hip):
    host = load_package().load_host()
    cfg, weights = model_setup(host)
    d = Dec(host, cfg, weights, 2)
    nan, inf = float("nan"), float("inf")
    for tau, eta in ((-1.0, 0.1), (32.5, 0.1), (nan, 0.1), (inf, 0.1), (5.0, 0.0), (5.0, -0.1), (5.0, 1.5), (5.0, nan), (5.0, inf)):
        assert d.o.set_mirostat_rc(0, tau, eta, None, 5) != 0, (tau, eta)
    for seq, mu, pos in ((2, None, 5), (-1, None, 5), (0, ref.MU_MAX + 1, 5), (0, -ref.MU_MAX - 1, 5), (0, None, 0), (0, None, cfg.max_ctx + 1)):
        assert d.o.set_mirostat_rc(seq, 5.0, 0.1, mu, pos) != 0, (seq, mu, pos)
    assert not d.o.mirostat_info()[3] and d.o.set_mirostat_rc(1, 0.0) == 0 and not d.o.mirostat_info()[3]      # clearing what was never set: nothing happens
    assert d.sampler_launches() == 0
    d.o.set_mirostat(1, 5.0, 0.1, None, 7)
    tq, eq, ps, on = d.o.mirostat_info()
    assert on and tq.tolist() == [0, 5 << 16] and eq.tolist() == [0, 6554] and ps.tolist() == [0, 7]
    assert d.o.mirostat_mus(1, 6, 3).tolist() == [0, 10 << 16, 0] and not d.o.mirostat_mus(0, 0, 16).any()      # the default start: 2 tau
    d.o.set_mirostat(1, 5.0, 0.1, -3, 8)
    assert d.o.mirostat_mus(1, 6, 3).tolist() == [0, 10 << 16, -3] and d.o.mirostat_info()[2].tolist() == [0, 8]
    assert d.sampler_launches() == 0                                   # a binding alone samples nothing: the greedy graph
    d.o.set_sampling(1, 40, 0.9, 1, 2)
    assert d.sampler_launches() >= 1
    # a cut and Mirostat on one sequence: whichever setter would create the pair
    assert d.o.set_cut_rc(1, 0.9, 0.0) != 0 and d.o.set_cut_rc(1, 1.0, 0.0) == 0 and d.o.set_cut_rc(0, 0.9, 0.1) == 0
    assert d.o.set_mirostat_rc(0, 5.0, 0.1, None, 5) != 0 and not d.o.mirostat_info()[0][0]
    assert d.o.set_cut_rc(0, 1.0, 0.0) == 0 and d.o.set_mirostat_rc(0, 5.0, 0.1, None, 5) == 0 and d.o.set_cut_rc(0, 0.5, 0.0) != 0
    for q in range(2):
        d.o.set_mirostat(q, 0.0)
    assert d.o.set_cut_rc(0, 0.5, 0.0) == 0 and d.o.set_cut_rc(0, 1.0, 0.0) == 0
    d.o.set_sampling(1, 0)
    assert d.sampler_launches() == 0 and d.o.mirostat_info()[3]
    d.o.close()
    # the single-sequence decoder: the same setter behind the model's handle
    m = weights_into(host.model(cfg), weights)
    assert m.set_mirostat_rc(40.0) != 0 and m.set_mirostat_rc(0.0) == 0 and not m.mirostat_info()[3]
    m.set_mirostat(3.0, 0.5, 7 << 16, 4)
    assert m.mirostat_info()[0].tolist() == [3 << 16] and m.mirostat_mus(4, 1).tolist() == [7 << 16] and m.set_cut_rc(0.9, 0.0) != 0
    m.set_mirostat(0.0)
    assert m.set_cut_rc(0.9, 0.0) == 0
    m.close()
