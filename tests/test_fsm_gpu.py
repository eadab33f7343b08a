"""-m gpu: token automata on the device (include/gten_hip_fsm.h, include/gten_host_fsm.h).

Everything here is an equality.  gten_hip_mask_rows_fsm is held to tests/fsm_ref.py bit for bit; gten_hip_sample_rows_fsm to the EXISTING
operators (sample_rows_biased / sample_rows_cut / sample_rows_pen) given the 0 / -inf bias row that restates the mask: the same id and
the same cut info bytes, because both sides run the same device code on a row with the same keys.  The decoder is held to the operator
on its own steps' logits with the host's copy of the state, and the host paths to the existing entry points' ids cut where the direct
scan says.

Not tested: the refusals on a persistent decoder (the product library is built without that step), a slot that moves between lanes in
the tail of a queue (it needs a queue through 256 slots; the binding is set again by the
same call that binds a slot in the first place), and the refusal of a pool above GTEN_HIP_FSM_MAX_BYTES on the device (no test uploads
a gigabyte; tests/test_fsm_cpu.py checks the arithmetic on the host)."""
import numpy as np
import pytest

import fsm_ref as ref
import penalty_ref as pref
from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from test_bias_gpu import NINF, SEED, Dec, P, upload
from test_logprobs_gpu import bits
from test_nucleus_gpu import model_setup

pytestmark = pytest.mark.gpu

VOCABS = [1, 2, 1023, 1024, 1025, 32003, 65535]
STATES = [0, 1, 2, 3, 4, -1, 1, 2]      # per row: four live states, the final one (4), unbound, and two states again with other logits


def rows_of(n_vocab, n_rows, seed):
    """logits with every sign: positive, negative, +0 (i % 7 == 3) and -0 (i % 7 == 5)"""
    g = np.random.default_rng(seed)
    x = (g.standard_normal((n_rows, n_vocab)) * 3.0).astype(np.float32)
    i = np.arange(n_vocab)
    x[:, i % 7 == 3] = 0.0
    x[:, i % 7 == 5] = -0.0
    return x


def pool_of(n_vocab, seed):
    """five states, the last final; live states allow about a quarter of the ids, with id 0 and the last id on both sides"""
    g = np.random.default_rng(seed)
    last = n_vocab - 1
    pin = [(0, 0, True), (0, last, True), (1, 0, False), (1, last, False), (2, 0, True), (2, last, False), (3, 0, False), (3, last, True)]
    if n_vocab == 1:
        pin = []
    elif n_vocab == 2:
        pin = [(0, 0, True), (0, 1, False), (1, 0, False), (1, 1, True), (2, 0, True), (2, 1, True), (3, 0, False), (3, 1, True)]
    return ref.random_pool(g, 5, n_vocab, 0.25, 1, pin)


# ------------------------------------------------------------------------------------------------------------ 1. the row

@pytest.mark.parametrize("n_vocab", VOCABS)
def test_mask_rows_equals_the_restatement_bit_for_bit(hip, n_vocab):
    nxt, flags = pool_of(n_vocab, n_vocab)
    assert hip.fsm_check(nxt, flags, n_vocab)[0] == 0
    pool = hip.fsm_upload(nxt, flags)
    R = len(STATES)
    x = rows_of(n_vocab, R, 3 * n_vocab)
    xb, stride = upload(hip, x, 3)
    y = hip.mask_rows_fsm(xb, R, n_vocab, stride, pool, STATES)
    for q, s in enumerate(STATES):
        want = ref.mask_row(x[q], nxt, flags, s)
        assert (bits(y[q]) == bits(want)).all(), (n_vocab, q, s)
        if s in (0, 1, 2, 3) and n_vocab >= 1023:
            banned = nxt[s] == ref.DEAD
            assert 0.6 < banned.mean() < 0.9 and (y[q][banned] == NINF).all()                  # about a quarter is allowed
            assert (bits(y[q][~banned]) == bits(x[q][~banned])).all()                            # allowed logits keep their bits, signed zeros too
    # a penalty in front: the penalised row, masked -- a ban stays a ban
    g = np.random.default_rng(n_vocab + 9)
    hist = [g.integers(0, n_vocab, L).astype(np.int32) for L in (0, 1, 300, 1025, 40, 7, 1024, 2)]
    r, f, p = np.full(R, 1.3, np.float32), np.linspace(-0.2, 0.5, R).astype(np.float32), np.full(R, 0.25, np.float32)
    r[3], f[3], p[3] = 1.0, 0.0, 0.0                                                             # one row without a penalty among them
    y = hip.mask_rows_fsm(xb, R, n_vocab, stride, pool, STATES, hist, r, f, p)
    for q, s in enumerate(STATES):
        want = ref.mask_row(pref.row(x[q], hist[q], r[q], f[q], p[q]), nxt, flags, s)
        assert (bits(y[q]) == bits(want)).all(), (n_vocab, q, s, "penalised")


def existing(hip, x, b, ks, temps, streams, pos, tp, mp, pen=None):
    """the ids (and cut info) of the operators that exist without automata on logits x under the bias rows b"""
    R, V = x.shape
    xb, bb = upload(hip, x)[0], upload(hip, b)[0]
    if pen is not None:
        hist, r, f, p = pen
        return hip.sample_rows_pen(xb, R, V, V, ks, temps, SEED, streams, pos, hist, r, f, p, tp, mp, bias=bb, bias_stride=V, info=True)
    cut, info = hip.sample_rows_cut(xb, R, V, V, ks, temps, SEED, streams, pos, tp, mp, bias=bb, bias_stride=V, info=True)
    if tp == 1.0 and mp == 0.0:
        assert hip.sample_rows_biased(xb, bb, R, V, V, V, ks, temps, SEED, streams, pos).tolist() == cut.tolist()
    return cut, info


@pytest.mark.parametrize("n_vocab", VOCABS)
def test_sample_rows_fsm_draws_what_the_existing_operators_draw_under_the_bias_that_restates_the_mask(hip, n_vocab):
    R = len(STATES)
    g = np.random.default_rng(n_vocab)
    streams = g.integers(0, 1 << 32, R, dtype=np.uint64).astype(np.uint32)
    pos = g.integers(1, 1 << 20, R).astype(np.int32)
    temps = np.array([0.7, 1.0, 1.5, 0.9, 1.0, 2.0, 0.8, 1.1], np.float32)
    nxt, flags = pool_of(n_vocab, n_vocab)
    # the seed of the logits is chosen on the existing operator alone: on at least a quarter of the rows its unmasked greedy winner is
    # an id the row's state bans (otherwise a mask that did nothing would pass)
    for seed in range(50):
        x = rows_of(n_vocab, R, 1000 * seed + n_vocab)
        free = hip.sample_rows(upload(hip, x)[0], R, n_vocab, n_vocab, 0, 1.0, SEED, streams, pos)
        moved = sum(1 for q, s in enumerate(STATES) if s in (0, 1, 2, 3) and nxt[s][free[q]] == ref.DEAD)
        if 4 * moved >= R or n_vocab == 1:
            break
    assert 4 * moved >= R or n_vocab == 1, "no seed found"
    pool = hip.fsm_upload(nxt, flags)
    xb, stride = upload(hip, x, 5)
    b = np.stack([ref.bias_of(nxt, flags, s, n_vocab) for s in STATES])
    want_next = lambda ids: [int(nxt[s][i]) if s in (0, 1, 2, 3) else s for s, i in zip(STATES, ids)]          # noqa: E731
    hist = [g.integers(0, n_vocab, L).astype(np.int32) for L in (5, 0, 300, 1025, 40, 7, 1, 64)]
    r, f, p = np.full(R, 1.2, np.float32), np.full(R, 0.1, np.float32), np.linspace(-0.3, 0.4, R).astype(np.float32)
    # 0: greedy; 1, 40: top-k; both sides of the 1024-candidate limit of the cut's two routines; the whole vocabulary
    for k in [0, 1, 40, 1023, 1024, 1025, n_vocab]:
        if k > n_vocab + 9:
            continue
        ks = np.full(R, k, np.int32)
        for tp, mp in [(1.0, 0.0), (0.9, 0.02), (0.5, 0.0)]:
            cut, info = existing(hip, x, b, ks, temps, streams, pos, tp, mp)
            got, after, ginfo = hip.sample_rows_fsm(xb, R, n_vocab, stride, pool, STATES, ks, temps, SEED, streams, pos, top_p=tp, min_p=mp, info=True)
            assert got.tolist() == cut.tolist() and ginfo.tobytes() == info.tobytes(), (n_vocab, k, tp, mp)
            assert after.tolist() == want_next(got), (n_vocab, k)                               # the next state is next[s][id]
            for q, s in enumerate(STATES):
                assert s not in (0, 1, 2, 3) or nxt[s][got[q]] != ref.DEAD, (n_vocab, k, q)      # never a banned id
        cut, info = existing(hip, x, b, ks, temps, streams, pos, 0.9, 0.01, (hist, r, f, p))
        got, after, ginfo = hip.sample_rows_fsm(xb, R, n_vocab, stride, pool, STATES, ks, temps, SEED, streams, pos, hist, r, f, p, 0.9, 0.01, info=True)
        assert got.tolist() == cut.tolist() and ginfo.tobytes() == info.tobytes() and after.tolist() == want_next(got), (n_vocab, k, "penalised")
    # a final row and an unbound one draw what the unmasked operator draws
    ks = np.array([0, 40, 1, 40, 40, 0, 40, n_vocab], np.int32)
    plain = hip.sample_rows(upload(hip, x)[0], R, n_vocab, n_vocab, ks, temps, SEED, streams, pos)
    got, after, _ = hip.sample_rows_fsm(xb, R, n_vocab, stride, pool, STATES, ks, temps, SEED, streams, pos)
    assert got[4] == plain[4] and got[5] == plain[5] and after[4] == 4 and after[5] == -1
    allp = hip.sample_rows_fsm(xb, R, n_vocab, stride, pool, [4, -1] * (R // 2), ks, temps, SEED, streams, pos)[0]
    assert allp.tolist() == plain.tolist()
    if n_vocab > 2:
        assert sum(int(a != b_) for a, b_ in zip(got.tolist(), plain.tolist())) >= 1               # the mask changed something


def test_a_pool_of_65535_states(hip):
    """n_vocab 2, every state index: state 65534, and the byte and half-word boundaries of an index"""
    V, S = 2, 65535
    s = np.arange(S)
    nxt = np.stack([(s * 7 + 1) % S, np.where(s % 2 == 0, ref.DEAD, (s + 255) % S)], 1).astype(np.uint16)
    flags = np.zeros(S, np.uint8)
    flags[[300, 65533]] = 1
    assert hip.fsm_check(nxt, flags, V)[0] == 0
    pool = hip.fsm_upload(nxt, flags)
    states = [0, 1, 254, 255, 256, 257, 300, 32767, 32768, 65533, 65534, 65279]
    R = len(states)
    x = np.tile(np.array([0.5, 2.0], np.float32), (R, 1))                                        # unmasked, id 1 wins
    xb = upload(hip, x)[0]
    y = hip.mask_rows_fsm(xb, R, V, V, pool, states)
    got, after, _ = hip.sample_rows_fsm(xb, R, V, V, pool, states, 0, 1.0, SEED, np.arange(R, dtype=np.uint32), np.full(R, 3, np.int32))
    for q, st in enumerate(states):
        assert (bits(y[q]) == bits(ref.mask_row(x[q], nxt, flags, st))).all(), st
        final = bool(flags[st])
        want = 1 if final or st % 2 == 1 else 0
        assert got[q] == want and after[q] == (st if final else int(nxt[st][want])), st
    assert after[states.index(65534)] == (65534 * 7 + 1) % S and got[states.index(65534)] == 0


def test_operator_argument_errors(hip):
    nxt, flags = pool_of(16, 1)
    pool = hip.fsm_upload(nxt, flags)
    xb = upload(hip, np.zeros(64))[0]
    ok = lambda **kw: hip.sample_rows_fsm(xb, 1, 16, 16, kw.pop("pool", pool), kw.pop("states", [0]), kw.pop("top_k", 40), 1.0, 0, 0, 1, **kw)     # noqa: E731
    ok()
    ok(states=[-1])
    ok(states=[4])
    pkg = load_package()
    for bad in (dict(states=[5]), dict(states=[-2]), dict(pool=(pool[0], pool[1], 0)), dict(pool=(pool[0], pool[1], 65536)), dict(top_k=-1),
                dict(top_p=0.0), dict(r=9.0, hist=[[1]])):
        with pytest.raises(pkg.GtenHipError):
            ok(**bad)


# ------------------------------------------------------------------------------------------------------------ 2. the decoder

TOTAL = 48                              # P prompt ids, the first new id from the prompt's logits, then 41 decode steps: a slice of 32 and a second one


def dec_pool(host, V):
    """two automata in one pool: A, twelve live states (nobody ever ends), and B, six states of which two are final"""
    pkg = load_package()
    g = np.random.default_rng(77)
    f = pkg.hostabi.Fsm(host, V)
    a = f.add_table(*ref.random_pool(g, 12, V, 0.25, 0))
    b = f.add_table(*ref.random_pool(g, 6, V, 0.25, 2))
    return f, a, b


def start_of(q, n_seq, a, b):
    """unbound on every third sequence, automaton A and B on the others in turn; a single sequence is in A"""
    if n_seq == 1:
        return a + 3
    return -1 if q % 3 == 0 else (a + q % 12 if q % 3 == 1 else b + q % 4)


def gen_fsm(d, prompts, total, starts, ks, streams, **kw):
    if d.one:
        ids, ended = d.o.generate_fsm(prompts[0], total, int(starts[0]), -1, int(ks[0]), 0.9, SEED, int(streams[0]), **kw)
        return [ids], np.array([ended])
    return d.o.generate_fsm(prompts, total, starts, -1, ks, 0.9, SEED, streams, **kw)


def dec_bind(d, q, state, pos=0):
    d.o.set_seq_fsm(state, pos) if d.one else d.o.set_seq_fsm(q, state, pos)


def dec_states(d, q, n_from, count):
    return d.o.fsm_states(n_from, count) if d.one else d.o.fsm_states(q, n_from, count)


@pytest.mark.parametrize("n_seq", [1, 2, 16, 256])
def test_decoder_follows_the_operator_and_the_walk(hip, n_seq):
    """the three step forms and, at 256, two lanes (the lane offsets of the bindings and of the state rows).  Bound and unbound
    sequences share the decoder; free-running generation (four steps per graph replay, a slice of 32 and a second slice) is, for a
    bound sequence, allowed id by allowed id the walk of its automaton, ends where the walk enters a final state, and is step by step
    the operator's id on the teacher-forced step's logits with the host's copy of the state"""
    host = load_package().load_host()
    cfg, weights = model_setup(host, 512)
    V = cfg.n_vocab
    d = Dec(host, cfg, weights, n_seq)
    prompts = [list(host.synthetic_tokens(P, seed=500 + q, n_vocab=V)) for q in range(n_seq)]
    streams = (np.arange(n_seq, dtype=np.uint32) * 3 + 1)
    ks = np.array([0 if q % 4 == 2 else 40 for q in range(n_seq)], np.int32)                     # greedy sequences among the sampling ones
    temps = np.full(n_seq, 0.9, np.float32)
    # every sequence before any binding: the parent's entry point
    parent = [d.o.generate_nucleus(prompts[0], TOTAL, -1, int(ks[0]), 0.9, SEED, int(streams[0]))] if d.one else \
        d.o.generate_nucleus(prompts, TOTAL, -1, ks, 0.9, SEED, streams)
    assert not d.o.fsm_info()[3] and d.o.fsm_info()[0] == 0
    f, a, b = dec_pool(host, V)
    nxt, flags = f.tables()
    d.o.set_fsm(f)
    assert d.o.fsm_info()[0] == f.n_states == 18 and not d.o.fsm_info()[3]
    starts = np.array([start_of(q, n_seq, a, b) for q in range(n_seq)], np.int32)
    nobody, ended0 = gen_fsm(d, prompts, TOTAL, np.full(n_seq, -1, np.int32), ks, streams)
    assert not d.o.fsm_info()[3] and not ended0.any()                                            # nobody bound: the rung is not taken
    got, ended = gen_fsm(d, prompts, TOTAL, starts, ks, streams)
    S, st, ps, on, _ = (*d.o.fsm_info(), None)
    assert on and (st == -1).all() and not ps.any()                                              # dropped afterwards
    moved = finals = 0
    for q in range(n_seq):
        assert nobody[q].tolist() == parent[q].tolist(), q
        new = got[q][P:].tolist()
        if starts[q] < 0:
            assert got[q].tolist() == parent[q].tolist() and ended[q] == 0, q                    # unbound beside bound ones: the parent's ids
            continue
        states = ref.walk(nxt, flags, starts[q], new)
        assert ref.DEAD not in states, q                                                         # every id was allowed where it was drawn
        end = ref.first_final(nxt, flags, starts[q], new)
        if end is None:
            assert len(got[q]) == TOTAL and ended[q] == 0, q
        else:
            assert end == len(new) - 1 and ended[q] == 2, q                                      # ends with the id that entered the final state
            finals += 1
        moved += new != parent[q][P:P + len(new)].tolist()
    assert moved >= 1 and (n_seq < 16 or finals >= 1)
    # teacher-forced, sequences of automaton A (which never end), against the operator on the step's own logits
    pool = hip.fsm_upload(nxt, flags)
    check = [q for q in range(n_seq) if starts[q] >= 0 and starts[q] < b and len(got[q]) == TOTAL]
    check = check if n_seq <= 16 else check[:6] + check[-6:]
    assert check and (n_seq < 256 or check[-1] >= 128)
    state = {}
    rows0 = {}
    for q in range(n_seq):
        d.request(q, int(ks[q]), 0.9, SEED, int(streams[q]))
        row = d.prefill(q, prompts[q])
        full = np.concatenate([got[q], np.zeros(TOTAL - len(got[q]), np.int32)])
        d.begin(q, full)
        if q in check:
            rows0[q] = row
    ids0, after0, _ = hip.sample_rows_fsm(upload(hip, np.stack([rows0[q] for q in check]))[0], len(check), V, V, pool, starts[check], ks[check],
                                          temps[check], SEED, streams[check], np.full(len(check), P, np.int32))
    assert ids0.tolist() == [int(got[q][P]) for q in check]                                      # the prompt's first id, drawn by the operator
    for i, q in enumerate(check):
        state[q] = int(after0[i])
        dec_bind(d, q, state[q], P + 1)
    S, st, ps, on, _ = (*d.o.fsm_info(), None)
    assert [int(st[q]) for q in check] == [state[q] for q in check] and all(ps[q] == P + 1 for q in check)
    assert d.sampler_launches() >= 1
    for n in range(P + 1, TOTAL):
        d.o.decode_step(n, use_graph=(n % 2 == 0))
        assert [d.result(q, n) for q in check] == [int(got[q][n]) for q in check], n
        rows = np.stack([d.logits(q) for q in check])
        ids, after, _ = hip.sample_rows_fsm(upload(hip, rows)[0], len(check), V, V, pool, [state[q] for q in check], ks[check], temps[check], SEED,
                                            streams[check], np.full(len(check), n, np.int32))
        assert ids.tolist() == [int(got[q][n]) for q in check], n
        for i, q in enumerate(check):
            assert dec_states(d, q, n, 2).tolist() == [state[q], int(after[i])], (q, n)         # the host's copy of the state, and the commit
            state[q] = int(after[i])
        if n in (P + 2, TOTAL - 2):
            d.o.decode_step(n, use_graph=(n % 2 == 1))                                           # a repeated step reads state[n], rewrites state[n + 1]
            assert [d.result(q, n) for q in check] == [int(got[q][n]) for q in check], n
            assert [int(dec_states(d, q, n + 1, 1)[0]) for q in check] == [state[q] for q in check]
    for q in check:
        assert dec_states(d, q, P + 1, TOTAL - P).tolist() == ref.walk(nxt, flags, starts[q], got[q][P:].tolist()), q
    # a rebind at a later position ignores what the row holds: the step at n0 draws in the state given, whatever state[n0] was
    n0 = P + 9
    q0 = check[-1]
    other = a + (int(dec_states(d, q0, n0, 1)[0]) - a + 5) % 12
    dec_bind(d, q0, other, n0)
    assert int(dec_states(d, q0, n0, 1)[0]) == other
    d.o.decode_step(n0, use_graph=True)
    row = d.logits(q0)
    i1, a1, _ = hip.sample_rows_fsm(upload(hip, row)[0], 1, V, V, pool, [other], ks[q0], 0.9, SEED, streams[q0], n0)
    assert d.result(q0, n0) == int(i1[0]) and dec_states(d, q0, n0, 2).tolist() == [other, int(a1[0])]
    # ... and a step before the binding's position is not looked at: position n0 - 1 draws unmasked
    d.o.decode_step(n0 - 1, use_graph=False)
    free = hip.sample_rows(upload(hip, d.logits(q0))[0], 1, V, V, ks[q0], 0.9, SEED, streams[q0], n0 - 1)
    assert d.result(q0, n0 - 1) == int(free[0]) and int(dec_states(d, q0, n0, 1)[0]) == other
    for q in range(n_seq):
        d.request(q, 0)
        dec_bind(d, q, -1)
    assert d.sampler_launches() == 0 and d.o.fsm_info()[3]
    f.close()
    d.o.close()


def test_the_refusals(hip):
    pkg = load_package()
    host = pkg.load_host()
    cfg, weights = model_setup(host)
    V = cfg.n_vocab
    d = Dec(host, cfg, weights, 2)
    assert d.o.set_seq_fsm_rc(0, 0, 5) != 0                                                      # no pool
    assert d.o.set_seq_fsm_rc(0, -1) == 0 and not d.o.fsm_info()[3]                              # unbinding what was never bound
    f, a, b = dec_pool(host, V)
    nxt, flags = f.tables()
    wrong = pkg.hostabi.Fsm(host, V + 1)
    wrong.add_stop([[1]])
    assert d.o.set_fsm_rc(wrong) != 0 and d.o.set_fsm_rc(pkg.hostabi.Fsm(host, V)) != 0          # another vocabulary; no state at all
    d.o.set_fsm(f)
    assert d.o.fsm_info()[0] == 18
    for seq, state, pos in ((2, 0, 5), (-1, 0, 5), (0, 18, 5), (0, -2, 5), (0, 0, 0), (0, 0, cfg.max_ctx + 1)):
        assert d.o.set_seq_fsm_rc(seq, state, pos) != 0, (seq, state, pos)
    assert not d.o.fsm_info()[3] and d.sampler_launches() == 0
    # a table and an automaton on one sequence: whichever setter would create the pair
    d.o.set_bias_table(0, [(1, NINF)])
    assert d.bind_rc(0, 0) == 0 and d.o.set_seq_fsm_rc(0, 3, 5) != 0
    assert d.o.set_seq_fsm_rc(1, 3, 5) == 0 and d.bind_rc(1, 0) != 0
    S, st, ps, on = d.o.fsm_info()
    assert on and st.tolist() == [-1, 3] and ps.tolist() == [0, 5] and d.sampler_launches() >= 1
    assert d.bind_rc(0, -1) == 0 and d.bind_rc(1, -1) == 0
    # while a sequence is bound the pool cannot be replaced, and the one in force stays
    small = pkg.hostabi.Fsm(host, V)
    small.add_stop([[1, 2]])
    assert d.o.set_fsm_rc(small) != 0 and d.o.set_fsm_rc(None) != 0 and d.o.fsm_info()[0] == 18
    api = pkg.hipabi.load()
    d.o.set_seq_fsm(1, -1)
    assert d.sampler_launches() == 0
    # what the upload's check refuses leaves the pool too: an entry outside the pool, a stuck state (through the raw tables)
    assert api.fsm_check(nxt, np.zeros(len(flags), np.uint8), V)[0] == 0
    bad = nxt.copy()
    bad[2, 7] = 18
    assert api.fsm_check(bad, flags, V)[0] == ref.BAD_ENTRY
    assert d.o.set_fsm_rc(small) == 0 and d.o.fsm_info()[0] == 3
    assert d.o.set_seq_fsm_rc(0, 3, 5) != 0 and d.o.set_seq_fsm_rc(0, 2, 5) == 0                 # the new pool's states
    d.o.set_seq_fsm(0, -1)
    assert d.o.set_fsm_rc(None) == 0 and d.o.fsm_info()[0] == 0 and d.o.set_seq_fsm_rc(0, 0, 5) != 0
    d.o.close()


def test_a_slot_that_repeats_its_last_step_leaves_the_walk(hip):
    """gten_hip_decoder_slot_start_until inside a free-running run of 32 shared steps, on a pool that masks every step: slot 0 reaches
    its last step after 11 steps and repeats it 21 times (DecStep::stop) while slot 1 runs on.  Every repeat reads the same state[last]
    and rewrites the same state[last + 1]: the state row equals the walk of the slot's ids, the entry behind it is untouched, and the
    ids are those of the same slot running on without a last step"""
    host = load_package().load_host()
    cfg, weights = model_setup(host, 512)
    V = cfg.n_vocab
    b = weights_into(host.batch(cfg, 2), weights)
    f, a, _ = dec_pool(host, V)
    nxt, flags = f.tables()
    b.set_fsm(f)
    pool = hip.fsm_upload(nxt, flags)
    prompts = [list(host.synthetic_tokens(P, seed=620 + q, n_vocab=V)) for q in range(2)]
    starts, streams = [a + 2, a + 7], np.array([4, 9], np.uint32)
    rows = np.stack([b.prefill(q, prompts[q]) for q in range(2)])
    id0, s1, _ = hip.sample_rows_fsm(upload(hip, rows)[0], 2, V, V, pool, starts, 40, 0.9, SEED, streams, P)
    dec = b.fsm_decoder()
    last0, steps = P + 11, 32

    def run(last):
        for q in range(2):
            b.decode_begin(q, prompts[q] + [int(id0[q])])
            b.set_sampling(q, 40, 0.9, SEED, int(streams[q]))
            b.set_seq_fsm(q, int(s1[q]), P + 1)
        hip.decoder_slot_start_until(dec, 0, P + 1, last)
        hip.decoder_slot_start_until(dec, 1, P + 1, 0)
        hip.decoder_run(dec, steps)
        n0 = (last or P + steps) - P
        return hip.decoder_slot_ids(dec, 0, P + 1, n0), hip.decoder_slot_ids(dec, 1, P + 1, steps)

    ids0, ids1 = run(last0)
    assert len(ids0) == 11
    st0, st1 = b.fsm_states(0, P + 1, 12), b.fsm_states(1, P + 1, steps + 1)
    walk0, walk1 = ref.walk(nxt, flags, int(s1[0]), ids0.tolist()), ref.walk(nxt, flags, int(s1[1]), ids1.tolist())
    assert ref.DEAD not in walk0 and ref.DEAD not in walk1                                       # every id was allowed where it was drawn
    assert st0.tolist() == [int(s1[0])] + walk0 and st1.tolist() == [int(s1[1])] + walk1
    assert int(st0[-1]) == int(nxt[st0[-2]][ids0[-1]])                                           # state[last + 1] = next[state[last]][id]
    assert int(b.fsm_states(0, last0 + 2, 1)[0]) == 0                                            # ... and nothing behind it was written
    free0, free1 = run(0)                                                                        # the same slot without a last step
    assert free0[:11].tolist() == ids0.tolist() and free1.tolist() == ids1.tolist()
    assert b.fsm_states(0, P + 1, 12).tolist() == st0.tolist()
    for q in range(2):
        hip.decoder_slot_park(dec, q)
        b.set_seq_fsm(q, -1)
        b.set_sampling(q, 0)
    b.close()
    f.close()


# ------------------------------------------------------------------------------------------------------------ 3. the ends

CUTS = (31, 32, 33)                     # generated indices at which a stop ends: either side of the first slice's edge (32 decode steps after the first id)
LEN = 56                                # ids in all: P + 50 new ones


def weights_into(o, weights):
    for i, w in enumerate(weights):
        o.set_weight(i, w)
    return o


def stops_for(new, V):
    """for one unconstrained answer `new` (generated ids): per cut in CUTS a two-id stop sequence whose first end, by the direct scan,
    is that index; None when this answer has no such pair for some cut"""
    out = []
    for c in CUTS:
        stop = [int(new[c - 1]), int(new[c])]
        if ref.stop_scan(new, [stop]) != c:
            return None
        out.append(stop)
    return out


def pick_seed(answers_of, V, tries=40):
    """the first seed, judged by the existing path's output alone, at which every answer has its three stops"""
    for seed in range(tries):
        answers = answers_of(seed)
        stops = [stops_for(a[P:].tolist(), V) for a in answers]
        if all(s is not None for s in stops):
            return seed, answers, stops
    raise AssertionError("no seed found")


def test_generate_fsm_with_a_stop_pool_on_a_model_and_a_batch(hip):
    pkg = load_package()
    host = pkg.load_host()
    cfg, weights = model_setup(host, 512, max_ctx=64)
    V = cfg.n_vocab
    m = weights_into(host.model(cfg), weights)
    prompts = [list(host.synthetic_tokens(P, seed=40 + j, n_vocab=V)) for j in range(2)]
    seed, (plain,), (stops,) = pick_seed(lambda s: [m.generate_topk(prompts[0], LEN, -1, 40, 1.0, s, 5)], V)
    new = plain[P:].tolist()
    never = next([i, i, i] for i in range(V) if ref.stop_scan(new, [[i, i, i]]) is None)
    f = pkg.hostabi.Fsm(host, V)
    start = {c: f.add_stop([stops[i], never]) for i, c in enumerate(CUTS)}          # (each with a second sequence that never occurs)
    s_never, s_first = f.add_stop([never]), f.add_stop([[new[0]], never])
    early = next(e for e in range(3, 16) if ref.stop_scan(new, [[new[e - 1], new[e]]]) == e)     # a stop that ends early in the first slice
    s_early = f.add_stop([[new[early - 1], new[early]]])
    nxt, flags = f.tables()
    m.set_fsm(f)
    for c in CUTS:
        ids, ended = m.generate_fsm(prompts[0], LEN, start[c], -1, 40, 1.0, seed, 5)
        assert ref.first_final(nxt, flags, start[c], new) == c                                   # the scan lands there
        assert ids.tolist() == plain[: P + c + 1].tolist() and ended == 2, c                     # cut just after the scan's position
        assert m.fsm_info()[1].tolist() == [-1]                                                  # no slot is bound afterwards
    ids, ended = m.generate_fsm(prompts[0], LEN, s_never, -1, 40, 1.0, seed, 5)
    assert ids.tolist() == plain.tolist() and ended == 0                                         # a stop that never occurs
    ids, ended = m.generate_fsm(prompts[0], LEN, s_first, -1, 40, 1.0, seed, 5)
    assert ids.tolist() == plain[: P + 1].tolist() and ended == 2                                # a first id that is itself final
    ids, ended = m.generate_fsm(prompts[0], LEN, -1, -1, 40, 1.0, seed, 5)
    assert ids.tolist() == plain.tolist() and ended == 0
    eos = new[10]
    at = new.index(eos)
    ids, ended = m.generate_fsm(prompts[0], LEN, start[32], eos, 40, 1.0, seed, 5)
    assert ids.tolist() == plain[: P + at].tolist() and ended == 1                               # the eos first: not kept
    ids, ended = m.generate_fsm(prompts[0], LEN, start[32], -1, 0)                               # greedy under a stop pool: greedy's ids, cut by the scan
    greedy = m.generate_biased(prompts[0], LEN, -1)
    end = ref.stop_scan(greedy[P:].tolist(), [stops[1], never])
    assert ids.tolist() == greedy[: LEN if end is None else P + end + 1].tolist() and ended == (0 if end is None else 2)
    assert m.fsm_info()[1].tolist() == [-1]
    # a binding at a later position over a row an ended sequence left behind: a run that ends early carries its final state on
    # through the rest of its slice, so the row holds final states from there to the slice's end.  Bound at generated index 25 --
    # in the middle of them -- through the setter, under an entry point that does not bind itself, the reader looks at nothing
    # before the binding: the automaton that never ends gives the full ids, the one whose stop ends at index 32 ends there
    ids, ended = m.generate_fsm(prompts[0], LEN, s_early, -1, 40, 1.0, seed, 5)
    assert ended == 2 and ids.tolist() == plain[: P + early + 1].tolist()
    stale = m.fsm_states(P + 1, 33)                                                              # state[P + 1 + i]: entered by generated id i
    assert all(flags[s] & 1 for s in stale[early:]) and not any(flags[s] & 1 for s in stale[:early]) and early < 24
    m.set_seq_fsm(s_never, P + 25)
    assert m.generate_topk(prompts[0], LEN, -1, 40, 1.0, seed, 5).tolist() == plain.tolist()
    m.set_seq_fsm(start[32], P + 25)
    assert m.generate_topk(prompts[0], LEN, -1, 40, 1.0, seed, 5).tolist() == plain[: P + 33].tolist()
    m.set_seq_fsm(-1)
    assert m.generate_topk(prompts[0], LEN, -1, 40, 1.0, seed, 5).tolist() == plain.tolist()
    with pytest.raises(pkg.GtenHipError):
        m.generate_fsm(prompts[0], LEN, f.n_states, -1, 40, 1.0, seed, 5)                        # a state outside the pool
    assert m.fsm_info()[1].tolist() == [-1]
    m.close()
    f.close()
    # a batch of 2: each sequence its own stops, in one pool
    b = weights_into(host.batch(cfg, 2), weights)
    seed, plain, stops = pick_seed(lambda s: b.generate_topk(prompts, LEN, -1, 40, 1.0, s, [3, 8]), V)
    f = pkg.hostabi.Fsm(host, V)
    start = [[f.add_stop([stops[q][i]]) for i in range(3)] for q in range(2)]
    first1 = f.add_stop([[int(plain[1][P])]])
    b.set_fsm(f)
    for i, c in enumerate(CUTS):
        other = CUTS[(i + 1) % 3]
        ids, ended = b.generate_fsm(prompts, LEN, [start[0][i], start[1][(i + 1) % 3]], -1, 40, 1.0, seed, [3, 8])
        assert ids[0].tolist() == plain[0][: P + c + 1].tolist() and ids[1].tolist() == plain[1][: P + other + 1].tolist() and ended.tolist() == [2, 2]
        assert (b.fsm_info()[1] == -1).all()
    ids, ended = b.generate_fsm(prompts, LEN, [-1, first1], -1, 40, 1.0, seed, [3, 8])
    assert ids[0].tolist() == plain[0].tolist() and ids[1].tolist() == plain[1][: P + 1].tolist() and ended.tolist() == [0, 2]
    with pytest.raises(pkg.GtenHipError):
        b.generate_fsm(prompts, LEN, [0, 0], -1, 40, 1.0, seed, [3, 8], tables=[0, -1])          # a table and an automaton on one sequence
    assert (b.fsm_info()[1] == -1).all()
    b.close()
    f.close()


@pytest.mark.parametrize("n_slots", [4, 16])
def test_serve_fsm_with_a_stop_pool(hip, n_slots):
    """a queue of n_slots + 5 prompts through n_slots slots in slices of 32 steps: every prompt its own stop, ending on either side
    of the slice edge, one that never ends and one whose first id is final; each answer is the existing path's, cut just after the
    scan's position.  (16 slots are held against the same-width decoder: its logits are not the single-sequence step's bit for bit.)"""
    pkg = load_package()
    host = pkg.load_host()
    cfg, weights = model_setup(host, 512, max_ctx=64)
    V = cfg.n_vocab
    n = n_slots + 5
    prompts = [list(host.synthetic_tokens(P + j % 3, seed=140 + j, n_vocab=V)) for j in range(n)]
    if n_slots < 16:
        m = weights_into(host.model(cfg), weights)
        alone = lambda s: [m.generate_topk(p, len(p) + 50, -1, 40, 1.0, s, j) for j, p in enumerate(prompts)]      # noqa: E731
    else:
        m = weights_into(host.batch(cfg, n_slots), weights)
        alone = lambda s: [m.generate_topk([p] * n_slots, len(p) + 50, -1, 40, 1.0, s, [j] * n_slots)[0] for j, p in enumerate(prompts)]      # noqa: E731
    for seed in range(40):                                    # (judged by the existing path's output alone)
        ans = alone(seed)
        stops = [stops_for(a[len(p):].tolist(), V) for a, p in zip(ans, prompts)]
        if all(s is not None for s in stops):
            break
    assert all(s is not None for s in stops), "no seed found"
    m.close()
    f = pkg.hostabi.Fsm(host, V)
    kind = [j % 5 for j in range(n)]                          # 0, 1, 2: a cut of CUTS; 3: never; 4: the first id
    starts, want = [], []
    for j in range(n):
        new = ans[j][len(prompts[j]):].tolist()
        if kind[j] < 3:
            starts.append(f.add_stop([stops[j][kind[j]]]))
            want.append(ans[j][: len(prompts[j]) + CUTS[kind[j]] + 1])
        elif kind[j] == 3:
            starts.append(f.add_stop([next([i, i, i] for i in range(V) if ref.stop_scan(new, [[i, i, i]]) is None)]))
            want.append(ans[j])
        else:
            starts.append(f.add_stop([[new[0]]]))
            want.append(ans[j][: len(prompts[j]) + 1])
    b = weights_into(host.batch(cfg, n_slots), weights)
    b.set_fsm(f)
    total = max(len(p) for p in prompts) + 50
    for sched in (1, 3):
        b.set_serve_schedule(sched)
        got, st, ended = b.serve_fsm(prompts, total, -1, 40, 1.0, seed, starts, slice_steps=32, max_new_each=[50] * n)
        assert st["admissions"] == n
        for j in range(n):
            assert got[j].tolist() == want[j].tolist(), (sched, j, kind[j])
            assert ended[j] == (0 if kind[j] == 3 else 2), (sched, j)
        assert (b.fsm_info()[1] == -1).all()
    # unbound prompts beside bound ones give the existing path's ids
    mixed = [s if j % 2 else -1 for j, s in enumerate(starts)]
    got, st, ended = b.serve_fsm(prompts, total, -1, 40, 1.0, seed, mixed, slice_steps=32, max_new_each=[50] * n)
    for j in range(n):
        assert got[j].tolist() == (want[j] if j % 2 else ans[j]).tolist() and ended[j] == (0 if (j % 2 == 0 or kind[j] == 3) else 2), j
    b.set_serve_schedule(0)
    assert (b.fsm_info()[1] == -1).all()
    b.close()
    f.close()


@pytest.mark.parametrize("n_seq", [1, 16])
def test_generate_fsm_with_a_choice_pool(hip, n_seq):
    pkg = load_package()
    host = pkg.load_host()
    cfg, weights = model_setup(host, 512, max_ctx=64)
    V = cfg.n_vocab
    g = np.random.default_rng(8)
    choices = [[7], [9, 300, 4], [9, 300, 5, 5], [9, 11], [400, 2, 2, 2, 2, 511], [0, 1]]
    f = pkg.hostabi.Fsm(host, V)
    start = f.add_choices(choices)
    d = Dec(host, cfg, weights, n_seq)
    d.o.set_fsm(f)
    prompts = [list(host.synthetic_tokens(P, seed=900 + q, n_vocab=V)) for q in range(n_seq)]
    seen = set()
    for seed in range(3):
        ks = np.array([40 if (q + seed) % 3 else 0 for q in range(n_seq)], np.int32)
        got, ended = gen_fsm(d, prompts, 40, np.full(n_seq, start, np.int32), ks, np.arange(n_seq, dtype=np.uint32) + 100 * seed)
        for q in range(n_seq):
            assert got[q][:P].tolist() == prompts[q] and got[q][P:].tolist() in choices and ended[q] == 2, (seed, q, got[q][P:].tolist())
            seen.add(tuple(got[q][P:].tolist()))
        assert (d.o.fsm_info()[1] == -1).all()
    assert n_seq == 1 or len(seen) >= 2
    # a choice longer than the room that is left is cut by the length, and says so
    got, ended = gen_fsm(d, prompts, P + 1, np.full(n_seq, start, np.int32), np.full(n_seq, 40, np.int32), np.arange(n_seq, dtype=np.uint32))
    for q in range(n_seq):
        assert len(got[q]) == P + 1 and ended[q] == (2 if got[q][P:].tolist() in choices else 0)
    f.close()
    d.o.close()
