"""-m gpu: sequences that are EXTENDED instead of recomputed (include/gten_host_sessions.h).  A sequence keeps the
K / V rows it has, the turn's ids become the positions behind them and only those rows go through the model.  Where the kept
rows came from the prompt path every comparison is byte or id EQUALITY with processing history + turn whole on the same
build; where decode steps wrote them, the logits are held to the oracle in the band of tests/test_multiseq_oracle_gpu.py."""
import numpy as np
import pytest

from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from helpers import F16, Q4, Q8, tiny_config
from test_model_gpu import check_logits, host_cfg

pytestmark = pytest.mark.gpu

MAX_CTX, N_SEQ = 384, 16                  # the batch of tests/test_prefix_gpu.py
WEIGHT_SEED = 777
_batches = {}


def batch_of(mode):
    """one 16-sequence batch per configuration for the whole module"""
    if mode not in _batches:
        wd, ad = {"q4": (Q4, Q8), "q8": (Q8, Q8), "f16": (F16, F16)}[mode]
        pkg = load_package()
        host = pkg.load_host()
        ocfg = tiny_config(wd, ad, n_heads=4, n_kv_heads=2, n_layers=2, max_ctx=MAX_CTX)
        cfg = host_cfg(ocfg)
        b = host.batch(cfg, N_SEQ)
        weights = [host.synth_weight(cfg, WEIGHT_SEED, i) for i in range(len(cfg.weight_shapes()))]
        for i, w in enumerate(weights):
            b.set_weight(i, w)
        _batches[mode] = (host, cfg, b, ocfg, weights)
    return _batches[mode]


@pytest.fixture(scope="module", autouse=True)
def _close_batches():
    yield
    for entry in _batches.values():
        entry[2].close()
    _batches.clear()


def toks(host, cfg, n, seed):
    return [int(t) for t in host.synthetic_tokens(n, seed=seed, n_vocab=cfg.n_vocab)]


def decode_after(b, host, cfg, prompts, steps=24):
    """`steps` ragged steps of every sequence on given ids behind prompts already in the caches of sequences 0 ..: (ids per
    step, last logits) -- the second half of tests/test_prefix_gpu.py's prefill_and_decode"""
    streams = [list(p) + toks(host, cfg, steps, 5000 + q) for q, p in enumerate(prompts)]
    streams += [toks(host, cfg, 4, 6000 + q) for q in range(len(prompts), N_SEQ)]
    for q, s in enumerate(streams):
        b.decode_begin(q, s)
    ids = []
    for t in range(1, steps + 1):
        ns = [len(p) + t for p in prompts] + [1] * (N_SEQ - len(prompts))
        b.decode_step_ragged(ns, use_graph=(t % 2 == 0))
        ids.append([b.decode_result(q, ns[q]) for q in range(len(prompts))])
    last = np.stack([b.logits(q) for q in range(len(prompts))])
    return ids, last


# heads: the boundary between kept and new rows inside a 16-lane column group (40), at a 256-position tile edge (256), inside a
# V sub-tile of the second tile (270); tails: full and partial row tiles, and one of 5 ids, a segment filled up to 16 rows
SPLITS = [(40, 16), (256, 17), (270, 33), (40, 50), (270, 16), (256, 50), (256, 5)]


@pytest.mark.parametrize("mode", ["q4", "f16"])
def test_extend_many_against_the_whole_prompts(hip, mode):
    host, cfg, b = batch_of(mode)[:3]
    whole = [toks(host, cfg, h + t, 1100 + i) for i, (h, t) in enumerate(SPLITS)]
    seqs = list(range(len(SPLITS)))
    want_lg = b.prefill_many(seqs, whole)
    want_ids, want_last = decode_after(b, host, cfg, whole)
    info0 = b.extend_info()
    b.prefill_many(seqs, [p[:h] for p, (h, _) in zip(whole, SPLITS)])
    got_lg, first = b.extend_many(seqs, [h for h, _ in SPLITS], [p[h:] for p, (h, _) in zip(whole, SPLITS)])
    info1 = b.extend_info()
    got_ids, got_last = decode_after(b, host, cfg, whole)
    # the short way WAS taken: one row matrix of the new rows
    assert tuple(x - y for x, y in zip(info1, info0)) == (len(SPLITS), sum(t for _, t in SPLITS), sum(h for h, _ in SPLITS), 0)
    for k, (h, t) in enumerate(SPLITS):
        d = np.abs(got_lg[k] - want_lg[k])
        print(f"{mode} head {h} tail {t}: turn logits differ in {int((d > 0).sum())} of {d.size}, max {float(d.max()):.4g}; "
              f"steps with other ids {sum(1 for a, w in zip(got_ids, want_ids) if a[k] != w[k])}; last logits max {float(np.abs(got_last[k] - want_last[k]).max()):.4g}")
    assert np.array_equal(got_lg, want_lg), ("turn logits", np.nonzero((got_lg != want_lg).any(axis=1))[0].tolist())
    assert first.tolist() == np.argmax(want_lg, axis=1).tolist()
    assert got_ids == want_ids, "ids of the decode steps that read the extended caches"
    assert np.array_equal(got_last, want_last), ("last step's logits", np.nonzero((got_last != want_last).any(axis=1))[0].tolist())


@pytest.mark.parametrize("mode", ["q4", "f16"])
def test_a_conversation_under_16_ids_goes_one_by_one(hip, oracle, mode):
    """8 ids, then 5 more: 13 ids are no prompt of the segmented path, so the turn's rows [8, 13) go through the sequence's own
    model object, operator by operator, beside two segments that go the short way.  Its logits against the oracle's logits of
    the 13 ids in the band of tests/test_multiseq_oracle_gpu.py (check_logits); the neighbours' bytes are the whole prompts'."""
    host, cfg, b, ocfg, weights = batch_of(mode)
    splits = [(40, 16), (8, 5), (270, 33)]
    whole = [toks(host, cfg, h + t, 1200 + i) for i, (h, t) in enumerate(splits)]
    seqs = [3, 4, 5]
    want_lg = b.prefill_many([3, 5], [whole[0], whole[2]])
    info0 = b.extend_info()
    b.prefill_many([3, 5], [whole[0][:40], whole[2][:270]])
    b.prefill(4, whole[1][:8], want=False)
    got_lg, first = b.extend_many(seqs, [h for h, _ in splits], [p[h:] for p, (h, _) in zip(whole, splits)])
    info1 = b.extend_info()
    assert tuple(x - y for x, y in zip(info1, info0)) == (2, 16 + 33, 40 + 270, 5)
    assert np.array_equal(got_lg[[0, 2]], want_lg)
    assert first.tolist() == np.argmax(got_lg, axis=1).tolist()
    om = oracle.model(ocfg)
    try:
        for i, w in enumerate(weights):
            om.set_weight(i, w)
        ref = om.logits(whole[1], 0)
    finally:
        om.close()
    rms, mx = check_logits(mode, got_lg[1], ref, float(ref.std()))
    print(f"{mode}: 5 rows one by one behind 8: rms {rms:.4g} max {mx:.4g} against the oracle")


@pytest.mark.parametrize("mode", ["q4", "f16"])
def test_extend_behind_rows_that_decode_steps_wrote(hip, oracle, mode):
    """200 prompt ids, 70 ragged steps on given ids (across position 256), then a turn of 20 ids as a continued segment: the
    context's rows 200 .. 269 are the decode path's.  The turn's logits against the oracle's logits of the whole 290 ids,
    in the band tests/test_multiseq_oracle_gpu.py holds this dtype and batch size to (check_logits)."""
    host, cfg, b, ocfg, weights = batch_of(mode)
    P, STEPS, TURN = 200, 70, 20
    watch = (0, 7)
    streams = [toks(host, cfg, P + STEPS + TURN, 1300 + q) for q in range(N_SEQ)]
    b.prefill_many(list(range(N_SEQ)), [s[:P] for s in streams])
    for q, s in enumerate(streams):
        b.decode_begin(q, s)
    for t in range(1, STEPS + 1):
        b.decode_step_ragged([P + t] * N_SEQ, use_graph=(t % 2 == 0))
    ctx = P + STEPS
    info0 = b.extend_info()
    got, _ = b.extend_many(list(watch), [ctx] * len(watch), [streams[q][ctx:] for q in watch])
    assert b.extend_info()[0] - info0[0] == len(watch)
    om = oracle.model(ocfg)
    try:
        for i, w in enumerate(weights):
            om.set_weight(i, w)
        for k, q in enumerate(watch):
            ref = om.logits(streams[q], 0)
            assert np.isfinite(got[k]).all()
            rms, mx = check_logits(mode, got[k], ref, float(ref.std()))
            print(f"{mode} sequence {q}: 20 rows behind 200 prompt + 70 decoded rows: rms {rms:.4g} max {mx:.4g} against the oracle")
    finally:
        om.close()


def test_extend_many_refusals(hip):
    host, cfg, b = batch_of("q4")[:3]
    t20 = toks(host, cfg, 20, 1400)
    b.prefill_many([0, 1], [toks(host, cfg, 40, 1401), toks(host, cfg, 40, 1402)])
    assert b.extend_many_rc([0, 0], [40, 40], [t20, t20]) == -1                     # a repeated sequence
    assert b.extend_many_rc([N_SEQ], [40], [t20]) == -1 and b.extend_many_rc([-1], [40], [t20]) == -1
    assert b.extend_many_rc([0], [0], [t20]) == -1                                  # nothing to continue: that is a prompt
    assert b.extend_many_rc([0], [40], [[]]) == -1                                  # an empty segment
    assert b.extend_many_rc([0], [MAX_CTX - 19], [t20]) == -1                       # ctx + rows = max_ctx + 1
    assert b.extend_many_rc([0, 1], [40, 40], [t20, t20[:3]]) == 0                  # taken: a segment and a short tail


# ---------------------------------------------------------------- sessions and serve_sessions

PROMPTS = (40, 64, 100, 17, 130, 30)          # turn 1
TURN2 = (20, 5, 33, 16, 1, 50)                # new ids of turn 2 (5 and 1: filled segments)
TURN3 = (8, 24, 3, 16, 40, 2)
NEW = 12                                      # ids generated per turn (eos -1: every turn runs to its bound)
PLAIN = (35, 16, 90)                          # plain prompts mixed into a queue


def conversation(host, cfg):
    return ([toks(host, cfg, n, 2100 + i) for i, n in enumerate(PROMPTS)], [toks(host, cfg, n, 2200 + i) for i, n in enumerate(TURN2)],
            [toks(host, cfg, n, 2300 + i) for i, n in enumerate(TURN3)], [toks(host, cfg, n, 2400 + i) for i, n in enumerate(PLAIN)])


def three_turns(b, host, cfg, schedule=0, spares=-1, mixed=False, reverse=False, **req):
    """three turns of six conversations through serve_sessions: (ids per turn and session, sessions_info before each turn and after)"""
    p1, u2, u3, plain = conversation(host, cfg)
    b.set_serve_schedule(schedule)
    b.set_serve_spares(spares)
    b.sessions_reserve(8)
    ss = [b.session_open() for _ in PROMPTS]
    out, infos = [], [b.sessions_info()]
    try:
        for turn in (p1, u2, u3):
            items = [(s, t) for s, t in zip(ss, turn)]
            if mixed:
                items = [x for pair in zip(items, [(None, p) for p in plain] + [None] * 3) for x in pair if x is not None]
            if reverse:
                items = items[::-1]
            ids, _, _ = b.serve_sessions(items, MAX_CTX, -1, req.get("top_k", 1), req.get("temp", 1.0), req.get("seed", 5),
                                         slice_steps=8, max_new=NEW)
            by_session = {s: ids[k] for k, (s, _) in enumerate(items) if s is not None}
            out.append([by_session[s].tolist() for s in ss])
            for s in ss:
                assert b.session_ids(s).tolist() == by_session[s].tolist()
                assert b.session_info(s)[:2] == (len(by_session[s]), len(by_session[s]) - 1)
            infos.append(b.sessions_info())
    finally:
        for s in ss:
            b.session_close(s)
        b.set_serve_schedule(0)
        b.set_serve_spares(-1)
    return out, infos


def greedy_steps(b, ids, count):
    """`count` greedy ids behind ids[q] (whose last id has no row yet) for sequences 0 .. len(ids) - 1, by ragged steps"""
    ids = [list(x) for x in ids]
    for _ in range(count):
        for q in range(N_SEQ):
            b.decode_begin(q, ids[q] if q < len(ids) else [1, 2, 3, 4])
        ns = [len(x) for x in ids] + [1] * (N_SEQ - len(ids))
        b.decode_step_ragged(ns, use_graph=False)
        for q in range(len(ids)):
            ids[q].append(b.decode_result(q, ns[q]))
    return ids


def manual_three_turns(b, host, cfg):
    """the same conversations by hand: prefill_many, then per turn extend_many behind the rows the sequence has and ragged greedy steps"""
    p1, u2, u3, _ = conversation(host, cfg)
    seqs = list(range(len(p1)))
    lg = b.prefill_many(seqs, p1)
    ids = [p + [int(np.argmax(lg[k]))] for k, p in enumerate(p1)]
    ids = greedy_steps(b, ids, NEW - 1)
    out = [[list(x) for x in ids]]
    for turn in (u2, u3):
        ctx = [len(x) - 1 for x in ids]                         # the last generated id has no row yet
        _, first = b.extend_many(seqs, ctx, [x[-1:] + t for x, t in zip(ids, turn)], want=False)
        ids = [x + t + [int(f)] for x, t, f in zip(ids, turn, first)]
        ids = greedy_steps(b, ids, NEW - 1)
        out.append([list(x) for x in ids])
    return out


def test_turn_one_is_serve_fsm(hip):
    host, cfg, b = batch_of("q4")[:3]
    p1 = conversation(host, cfg)[0]
    for top_k, temp in ((1, 1.0), (8, 0.9)):
        want, _, want_end = b.serve_fsm(p1, MAX_CTX, -1, top_k, temp, 5, -1, slice_steps=8, max_new=NEW)
        got, _ = three_turns(b, host, cfg, top_k=top_k, temp=temp)
        assert got[0] == [w.tolist() for w in want], (top_k, temp)


def test_turns_two_and_three_whatever_the_queue(hip):
    host, cfg, b = batch_of("q4")[:3]
    want = manual_three_turns(b, host, cfg)
    base, infos = three_turns(b, host, cfg, schedule=1, spares=0)
    assert base == want, "serve_sessions against extend_many + ragged steps by hand"
    # the continued turns were taken, and each computed its new ids and the one id of the history that had no row
    for turn, new in ((1, TURN2), (2, TURN3)):
        d = tuple(x - y for x, y in zip(infos[turn + 1][2:], infos[turn][2:]))
        hist = sum(len(x) for x in want[turn - 1])
        assert d == (len(new), len(new), sum(n + 1 for n in new), hist - len(new)), (turn, d)
    assert infos[1][2:4] == (infos[0][2] + len(PROMPTS), infos[0][3])          # turn 1: whole prompts
    for kw in (dict(schedule=3, spares=-1), dict(schedule=1, spares=-1, mixed=True), dict(schedule=3, spares=0, mixed=True, reverse=True)):
        got, _ = three_turns(b, host, cfg, **kw)
        assert got == want, kw
    wide = host.batch(cfg, 32)
    try:
        for i, w in enumerate(batch_of("q4")[4]):
            wide.set_weight(i, w)
        got, _ = three_turns(wide, host, cfg, schedule=3, spares=-1, mixed=True)
        assert got == want, "32 slots"
        got, _ = three_turns(wide, host, cfg, schedule=1, spares=0)
        assert got == want, "32 slots, sessions alone, no spares"
    finally:
        wide.close()


def test_truncate_and_an_empty_turn_regenerate_the_answer(hip):
    host, cfg, b = batch_of("q4")[:3]
    p1, u2, _, _ = conversation(host, cfg)
    b.sessions_reserve(8)
    s = b.session_open()
    try:
        b.serve_sessions([(s, p1[2])], MAX_CTX, -1, 1, 1.0, 5, max_new=NEW)
        ids2, _, _ = b.serve_sessions([(s, u2[2])], MAX_CTX, -1, 1, 1.0, 5, max_new=NEW)
        asked = len(ids2[0]) - NEW                              # the end of the user's turn
        b.session_truncate(s, asked)
        assert b.session_info(s)[:2] == (asked, asked)
        again, _, _ = b.serve_sessions([(s, [])], MAX_CTX, -1, 1, 1.0, 5, max_new=NEW)
        assert again[0].tolist() == ids2[0].tolist()
        assert b.session_truncate_rc(s, len(again[0]) + 1) == -1 and b.session_truncate_rc(s, -1) == -1
    finally:
        b.session_close(s)


def test_a_session_behind_a_registered_prefix(hip):
    """The prefix mark of a session's set outlives the queue: turn 2's slot start renews the promise, so the slot reads the prefix's
    full chunk (256 positions) from the decoder's one copy and its import skips that chunk -- read from the decoder's cumulative
    counter of imports that skipped shared chunks (prefix_decode_info), before and after each queue, as
    tests/test_prefix_decode_gpu.py does.  With the switch off nobody skips; with the prefix replaced between the turns the mark is
    gone and turn 2 skips nothing.  The ids are the same all three ways."""
    host, cfg, b = batch_of("q4")[:3]
    P = 256                                                   # one full chunk: 256 + 30 + 12 + 20 + 12 ids fit max_ctx 384
    pre, other = toks(host, cfg, P, 2500), toks(host, cfg, P, 2501)
    prompt, turn = pre + toks(host, cfg, 30, 2502), toks(host, cfg, 20, 2503)
    b.sessions_reserve(8)
    runs, skipped = {}, {}

    def skips():
        return b.prefix_decode_info()[3]

    try:
        for how in ("shared", "own copy", "replaced"):
            host.set_prefix_decode_shared(how != "own copy")
            b.set_prefix_at(1, pre)
            s = b.session_open()
            try:
                sk0 = skips()
                first, _, _ = b.serve_sessions([(s, prompt)], MAX_CTX, -1, 1, 1.0, 5, max_new=NEW)
                sk1 = skips()
                assert b.session_info(s)[2:] == (1, P), "the first turn took the short way and the set keeps the mark"
                if how == "replaced":
                    b.set_prefix_at(1, other)
                    assert b.session_info(s)[2:] == (-1, 0), "a replaced prefix takes the mark along"
                sk1b = skips()
                second, _, _ = b.serve_sessions([(s, turn)], MAX_CTX, -1, 1, 1.0, 5, max_new=NEW)
                sk2 = skips()
                if how != "replaced":
                    assert b.session_info(s)[2:] == (1, P), "the turn wrote rows behind the prefix only"
                runs[how] = (first[0].tolist(), second[0].tolist())
                skipped[how] = (sk1 - sk0, sk2 - sk1b)
            finally:
                b.session_close(s)
    finally:
        host.set_prefix_decode_shared(None)
        b.set_prefix_at(1, None)
    print("imports that skipped the shared chunk (turn 1, turn 2):", skipped)
    assert runs["shared"] == runs["own copy"] == runs["replaced"]
    assert len(runs["shared"][1]) == P + 30 + NEW + 20 + NEW
    # turn 2 of the session started ONCE on a slot that shared the prefix's chunk: the mark was still on its set and was renewed
    assert skipped["shared"] == (1, 1), skipped
    assert skipped["own copy"] == (0, 0), skipped
    assert skipped["replaced"] == (1, 0), skipped


def test_serve_sessions_return_codes(hip):
    host, cfg = batch_of("q4")[:2]
    t20 = toks(host, cfg, 20, 2600)
    b = host.batch(cfg, N_SEQ)                                                      # (a batch of its own: two sessions reserved, no more)
    for i, w in enumerate(batch_of("q4")[4]):
        b.set_weight(i, w)
    b.sessions_reserve(2)
    assert b.host._bsess_reserve(b.h, 257) == -1 and b.host._bsess_reserve(b.h, -1) == -1
    s = b.session_open()
    other = b.session_open()
    try:
        with pytest.raises(load_package().GtenHipError):
            b.session_open()                                                        # both reserved sessions are open
        assert b.serve_sessions_rc([(s, t20), (s, t20)], MAX_CTX, -1, 1, 1.0, 5, max_new=4)[0] == -1        # the same session twice
        assert b.serve_sessions_rc([(7, t20)], MAX_CTX, -1, 1, 1.0, 5, max_new=4, stride=MAX_CTX)[0] == -1  # not a session
        assert b.serve_sessions_rc([(s, [])], MAX_CTX, -1, 1, 1.0, 5, max_new=4)[0] == -1                   # nothing to take logits from
        assert b.serve_sessions_rc([(s, t20)], MAX_CTX, -1, 1, 1.0, 5, max_new=4)[0] == 0
        assert b.session_info(s)[:2] == (24, 23)
        assert b.serve_sessions_rc([(s, t20)], 30, -1, 1, 1.0, 5, max_new=4, stride=30)[0] == -1            # 44 ids do not fit a stride of 30
        assert b.session_info(s)[:2] == (24, 23)
        # no room to generate: returned as it is, the session unchanged
        rc, ids, _, _ = b.serve_sessions_rc([(s, t20)], 40, -1, 1, 1.0, 5, stride=64)
        assert rc == 0 and len(ids[0]) == 44 and b.session_info(s)[:2] == (24, 23)
        b.session_close(other)
        assert b.serve_sessions_rc([(other, t20)], MAX_CTX, -1, 1, 1.0, 5, max_new=4, stride=MAX_CTX)[0] == -1   # closed
        again = b.session_open()
        assert again == other and b.session_info(again)[:2] == (0, 0)
        b.session_close(again)
        assert b.sessions_info()[0] == 1
    finally:
        b.close()


def test_penalties_and_a_stop_automaton_on_a_session_item(hip):
    """A first turn that generates ONE id leaves a history whose rows are all the prompt path's, so the second turn's rows are the
    whole prompt's byte for byte: the request on the session item must give the ids of the same request on the written-out history
    -- the penalty window, the automaton's position and the sampler's noise all speak of the history's positions."""
    pkg = load_package()
    host, cfg, b = batch_of("q4")[:3]
    p1, u2, _, _ = conversation(host, cfg)
    f = pkg.hostabi.Fsm(host, cfg.n_vocab)
    b.sessions_reserve(8)
    ss = [b.session_open() for _ in range(3)]
    req = dict(rep=1.3, freq=0.2, pres=0.1, last_n=64, slice_steps=8, max_new=NEW)
    try:
        first, _, _ = b.serve_sessions([(s, p1[k]) for k, s in enumerate(ss)], MAX_CTX, -1, 8, 0.9, 11, max_new=1)
        whole = [first[k].tolist() + u2[k] for k in range(3)]
        free, _, _ = b.serve_fsm(whole, MAX_CTX, -1, 8, 0.9, 11, -1, **req)
        # a stop sequence that the free run of item 0 produces at its 4th and 5th new ids
        stop = [int(x) for x in free[0][len(whole[0]) + 3:len(whole[0]) + 5]]
        start = f.add_stop([stop])
        b.set_fsm(f)
        starts = [start, -1, start]
        want, _, want_end = b.serve_fsm(whole, MAX_CTX, -1, 8, 0.9, 11, starts, **req)
        got, _, got_end = b.serve_sessions([(s, u2[k]) for k, s in enumerate(ss)], MAX_CTX, -1, 8, 0.9, 11, fsm_start=starts, **req)
        assert [g.tolist() for g in got] == [w.tolist() for w in want]
        assert got_end.tolist() == want_end.tolist() and len(want[0]) == len(whole[0]) + 5
    finally:
        for s in ss:
            b.session_close(s)
