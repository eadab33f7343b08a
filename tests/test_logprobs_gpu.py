"""-m gpu: the log-prob of every generated id and its top-N alternatives on the device (include/gten_hip_logprobs.h,
include/gten_host_logprobs.h).

The operator is held to tests/logprobs_ref.py: the ids exactly, the log-probs within 1e-4 + 1e-6 |value| (the bound
tests/test_score_gpu.py holds gten_hip_row_logprobs to).  The decoder's records are held to the operator on its own steps' logits,
bit for bit; the serving queue to generating each prompt alone; and asking changes no id anywhere."""
import numpy as np
import pytest

import bias_ref as bref
import logprobs_ref as ref
from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from test_bias_gpu import NINF, POISON, SEED, TOTAL, Dec, P, model_setup, upload

pytestmark = pytest.mark.gpu

VOCABS = [1, 63, 64, 1000, 32003]
N_TOPS = [0, 1, 5, 20]
ROWS = 5


def close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool((np.abs(got - want) <= 1e-4 + 1e-6 * np.abs(want)).all())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_rows(x, chosen, n_top, lp, ti, tl):
    """the operator's outputs for rows x against the restatement"""
    for r in range(len(x)):
        wlp, wid, wtl = ref.record(x[r], n_top, int(chosen[r]))
        print(f"row {r}: n_vocab {x.shape[1]} n_top {n_top} logprob {lp[r]:.6f} (ref {wlp:.6f}) max |top diff| "
              f"{np.abs(tl[r] - wtl).max() if n_top else 0.0:.2e}")
        assert ti[r].tolist() == wid.tolist(), (r, n_top)
        assert close(lp[r], wlp) and close(tl[r], wtl), (r, n_top, lp[r], wlp)
        if chosen[r] < 0:
            assert bits(lp[r]) == 0
        hit = np.flatnonzero(ti[r] == chosen[r]) if chosen[r] >= 0 else []
        if len(hit):
            assert bits(tl[r][hit[0]]) == bits(lp[r]), (r, n_top)           # the chosen id's entry: the same bits


@pytest.mark.parametrize("n_vocab", VOCABS)
def test_operator_follows_the_restatement(hip, n_vocab):
    r = np.random.default_rng(n_vocab)
    x = (r.standard_normal((ROWS, n_vocab)) * 3.0).astype(np.float32)
    x[1] = (np.round(x[1] * 2.0) / 2.0).astype(np.float32)                  # a grid: many ties
    chosen = np.array([int(np.argmax(x[0])), n_vocab - 1, -1, int(r.integers(n_vocab)), 0], np.int32)
    xb, stride = upload(hip, x, 5)                                          # poisoned padding between the rows
    for n_top in N_TOPS:
        lp, ti, tl = hip.row_top_logprobs(xb, ROWS, n_vocab, stride, chosen, n_top)
        assert ti.shape == (ROWS, n_top) and tl.shape == (ROWS, n_top)
        check_rows(x, chosen, n_top, lp, ti, tl)
        if n_top:
            assert [hip.argmax_row(xb, n_vocab, 4 * stride * q) for q in range(ROWS)] == ti[:, 0].tolist()
        # gten_hip_row_logprobs' rank of the chosen id is below n_top exactly when the id is in the list
        scored = np.where(chosen >= 0, chosen, 0).astype(np.int32)
        slp, rank, _ = hip.row_logprobs(xb, ROWS, n_vocab, stride, scored)
        lp2, ti2, _ = hip.row_top_logprobs(xb, ROWS, n_vocab, stride, scored, n_top)
        for q in range(ROWS):
            assert (rank[q] < n_top) == (scored[q] in ti2[q].tolist()), (q, n_top, rank[q])
            assert rank[q] == ref.rank(x[q], scored[q])
            assert close(lp2[q], slp[q])


def test_operator_ties_at_the_cut_all_equal_and_signed_zeros(hip):
    n = 1000
    # three distinct values: 7 ids at 5, a run of 40 at 2, the rest at -3
    x = np.full(n, -3.0, np.float32)
    high = [3, 77, 400, 401, 650, 900, 999]
    run = list(range(100, 120)) + list(range(500, 520))
    x[high] = 5.0
    x[run] = 2.0
    xb = upload(hip, x)[0]
    for n_top in (1, 5, 7, 8, 12, 20):
        _, ti, tl = hip.row_top_logprobs(xb, 1, n, n, -1, n_top)
        assert ti[0].tolist() == (high + run)[:n_top], n_top
        check_rows(x[None], [-1], n_top, [0.0], ti, tl)
    # the cut inside the lowest value's run, and past 256 equal values (the second select's second digit)
    y = np.full(n, 1.5, np.float32)
    yb = upload(hip, y, 3)[0]
    for n_top in (1, 5, 20):
        lp, ti, tl = hip.row_top_logprobs(yb, 1, n, n + 3, 999, n_top)
        assert ti[0].tolist() == list(range(n_top))
        assert close(lp, -np.log(float(n))) and close(tl, np.full(n_top, -np.log(float(n))))
    z = np.full(n, -1.0, np.float32)
    z[300:] = np.where(np.arange(n - 300) % 2 == 0, -0.0, 0.0).astype(np.float32)     # -0 / +0 alternate from 300 on: one value
    assert np.signbit(z[300]) and not np.signbit(z[301])
    zb = upload(hip, z)[0]
    _, ti, _ = hip.row_top_logprobs(zb, 1, n, n, -1, 20)
    assert ti[0].tolist() == list(range(300, 320))
    # fewer ids than alternatives
    w = np.array([0.5, 2.0, 1.0], np.float32)
    lp, ti, tl = hip.row_top_logprobs(upload(hip, w)[0], 1, 3, 3, 1, 5)
    assert ti[0].tolist() == [1, 2, 0, -1, -1] and tl[0][3:].tolist() == [0.0, 0.0] and bits(lp[0]) == bits(tl[0][0])


def test_operator_argument_errors(hip):
    xb = upload(hip, np.zeros(64))[0]
    rc = lambda n_rows, n_vocab, stride, n_top: hip.row_top_logprobs_rc(xb, n_rows, n_vocab, stride, n_top)      # noqa: E731
    assert rc(1, 16, 16, 5) == 0
    hip.sync()
    assert rc(1, 0, 16, 5) != 0 and rc(1, 16, 15, 5) != 0 and rc(0, 16, 16, 5) != 0 and rc(65536, 16, 16, 5) != 0
    assert rc(1, 16, 16, -1) != 0 and rc(1, 16, 16, 21) != 0
    assert rc(1, 16, 16, 0) == 0 and rc(4, 16, 16, 20) == 0
    hip.sync()


# ------------------------------------------------------------------------------------------------------------ the decoder

def mixed(n_seq, shift):
    """per sequence: top_k (0 / 40), n_top (-1 / 0 / 3 / 20), table (-1 / 1)"""
    ks = np.array([0 if (q + shift) % 2 == 0 else 40 for q in range(n_seq)], np.int32)
    tops = np.array([(-1, 0, 3, 20)[((q + shift) // 2) % 4] for q in range(n_seq)], np.int32)
    tables = np.array([1 if (q + shift) % 8 in (4, 5, 6, 7) else -1 for q in range(n_seq)], np.int32)
    return ks, tops, tables


def dec_ask(d, q, n_top):
    d.o.set_logprobs(int(n_top)) if d.one else d.o.set_logprobs(q, int(n_top))


def dec_records(d, q, n_from, count, n_top):
    return d.o.logprobs(n_from, count, n_top) if d.one else d.o.logprobs(q, n_from, count, n_top)


def dec_generate_lp(d, prompts, total, tops, ks, temps, seed, streams, tables):
    """(ids per sequence, logprob [n_seq][total], top_id [n_seq][total][20], top_logprob)"""
    if d.one:
        if tops[0] < 0:
            ids = d.o.generate_biased(prompts[0], total, -1, int(ks[0]), float(temps[0]), seed, int(streams[0]), int(tables[0]), 0)
            return [ids], np.zeros((1, total), np.float32), np.full((1, total, 20), -1, np.int32), np.zeros((1, total, 20), np.float32)
        ids, lp, ti, tl = d.o.generate_logprobs(prompts[0], total, int(tops[0]), -1, int(ks[0]), float(temps[0]), seed, int(streams[0]), int(tables[0]), 0)
        ti20, tl20 = np.full((1, total, 20), -1, np.int32), np.zeros((1, total, 20), np.float32)
        ti20[0, :, : tops[0]], tl20[0, :, : tops[0]] = ti, tl
        return [ids], lp[None], ti20, tl20
    ids, lp, ti, tl = d.o.generate_logprobs(prompts, total, tops, -1, ks, temps, seed, streams, tables, None)
    ti20, tl20 = np.full((d.n, total, 20), -1, np.int32), np.zeros((d.n, total, 20), np.float32)
    ti20[:, :, : ti.shape[2]], tl20[:, :, : tl.shape[2]] = ti, tl
    return ids, lp, ti20, tl20


@pytest.mark.parametrize("n_seq", [1, 2, 16, 128])
def test_decoder_records_equal_the_operator_on_its_own_logits(hip, n_seq):
    host = load_package().load_host()
    cfg, weights = model_setup(host)
    V = cfg.n_vocab
    d = Dec(host, cfg, weights, n_seq)
    assert d.sampler_launches() == 0
    prompts = [list(host.synthetic_tokens(P, seed=700 + q, n_vocab=V)) for q in range(n_seq)]
    streams = (np.arange(n_seq, dtype=np.uint32) * 3 + 1)
    temps = np.full(n_seq, 0.9, np.float32)
    zero = np.zeros(n_seq, np.int32)
    none = np.full(n_seq, -1, np.int32)
    greedy = d.generate(prompts, TOTAL, zero, temps, SEED, streams, none, zero)
    # the table bans each sequence's natural first ids: the greedy run's ids at the first three new positions
    banned = sorted({int(g[p]) for g in greedy for p in (P, P + 1, P + 2)})[: V // 2]
    d.o.set_bias_table(1, [(j, NINF) for j in banned])
    table = bref.table(V, [(j, NINF) for j in banned])
    check = list(range(n_seq)) if n_seq <= 16 else [q for q in range(n_seq) if q % 16 < 4 or q % 16 >= 12]
    saw_banned_first = 0
    for shift in (range(8) if n_seq == 1 else (1, 5) if n_seq == 2 else (0,)):
        ks, tops, tables = mixed(n_seq, shift)
        # 1. asking changes no id
        want = d.generate(prompts, TOTAL, ks, temps, SEED, streams, tables, zero)
        got, lp, ti, tl = dec_generate_lp(d, prompts, TOTAL, tops, ks, temps, SEED, streams, tables)
        for q in range(n_seq):
            assert got[q].tolist() == want[q].tolist(), (shift, q)
            if tops[q] < 0:
                assert not lp[q].any() and (ti[q] == -1).all() and not tl[q].any(), (shift, q)
            else:
                assert not lp[q][:P].any() and (ti[q][:P] == -1).all() and (ti[q][:, tops[q]:] == -1).all()        # prompt positions, entries past n_top
        # 2. the host-driven loop, teacher-forced with those ids: every step's record against the operator on that step's logits
        rows0 = []
        for q in range(n_seq):
            d.request(q, int(ks[q]), 0.9, SEED, int(streams[q]))
            assert d.bind_rc(q, int(tables[q])) == 0
            dec_ask(d, q, tops[q])
            rows0.append(d.prefill(q, prompts[q]))
            d.begin(q, got[q])
        assert (d.sampler_launches() >= 1) == bool((ks > 0).any() or (tables >= 0).any() or (tops >= 0).any())
        asking = [q for q in check if tops[q] >= 0]

        def against_operator(rows, n, qs):
            for q, row in zip(qs, rows):
                olp, oti, otl = hip.row_top_logprobs(upload(hip, row)[0], 1, V, V, int(got[q][n]), int(tops[q]))
                # the generation call's outputs at this position: the same bits
                assert bits(lp[q][n]) == bits(olp[0]), (shift, q, n, lp[q][n], olp[0])
                assert ti[q][n][: tops[q]].tolist() == oti[0].tolist() and (bits(tl[q][n][: tops[q]]) == bits(otl[0])).all(), (shift, q, n)
                yield q, olp[0], oti[0], otl[0]

        n_first_banned = 0
        for q, olp, oti, otl in against_operator([rows0[q] for q in asking], P, asking):          # the first new id: from the prompt's logits
            if tops[q] > 0:
                if ks[q] == 0 and tables[q] < 0:
                    assert oti[0] == got[q][P]
                if tables[q] >= 0 and int(np.argmax(rows0[q])) in banned:
                    assert oti[0] == int(np.argmax(rows0[q])) and got[q][P] != oti[0]
                    n_first_banned += 1
        saw_banned_first += n_first_banned
        for n in range(P + 1, TOTAL):
            d.o.decode_step(n)
            assert [d.result(q, n) for q in range(n_seq)] == [int(g[n]) for g in got], (shift, n)
            rows = [d.logits(q) for q in asking]
            for (q, olp, oti, otl), row in zip(against_operator(rows, n, asking), rows):
                rlp, rti, rtl = dec_records(d, q, n, 1, int(tops[q]))                               # this step's record: the same bits again
                assert bits(rlp[0]) == bits(olp) and rti[0].tolist() == oti.tolist() and (bits(rtl[0]) == bits(otl)).all(), (shift, q, n)
                wlp, wid, wtl = ref.record(row, int(tops[q]), int(got[q][n]))
                assert close(olp, wlp) and oti.tolist() == wid.tolist() and close(otl, wtl)
                if tops[q] > 0:
                    if ks[q] == 0 and tables[q] < 0:
                        assert oti[0] == got[q][n]                                                   # greedy, unbound: the id is the first alternative
                    if tables[q] >= 0:
                        assert oti[0] == int(np.argmax(row))                                         # raw logits: a banned maximum is still listed first
                        assert table[got[q][n]] > NINF
        for q in range(n_seq):
            d.request(q, 0)
            assert d.bind_rc(q, -1) == 0
            dec_ask(d, q, -1)
        assert d.sampler_launches() == 0                                                             # nobody asks: the greedy graph again
    assert saw_banned_first >= 1
    again = d.generate(prompts, TOTAL, zero, temps, SEED, streams, none, zero)
    assert all(a.tolist() == g.tolist() for a, g in zip(again, greedy))
    d.o.close()


def test_requests_are_checked_and_read_back(hip):
    host = load_package().load_host()
    cfg, weights = model_setup(host)
    d = Dec(host, cfg, weights, 2)
    assert d.o.set_logprobs_rc(0, 21) != 0 and d.o.set_logprobs_rc(0, -2) != 0 and d.o.set_logprobs_rc(2, 3) != 0
    with pytest.raises(load_package().GtenHipError):
        d.o.logprobs(0, 1, 1, 3)                                          # no sequence has asked yet: no records
    d.o.set_logprobs(1, 7)
    lp, ti, tl = d.o.logprobs(1, 0, 66, 20)                               # every position of the buffer, before any step: zeroed
    assert not lp.any() and not ti.any() and not tl.any()
    d.o.set_sampling(1, 40, 0.9, 1, 2)                                    # the other halves of the request leave it alone
    d.o.set_seq_bias(1, 0, 0)
    assert d.sampler_launches() >= 1
    d.o.set_sampling(1, 0)
    d.o.set_seq_bias(1, -1)
    assert d.sampler_launches() >= 1                                      # sequence 1 still asks
    d.o.set_logprobs(1, -1)
    assert d.sampler_launches() == 0
    d.o.close()


# ---------------------------------------------------------------------------------------------------------------- serving

def sampler_launches(o, n=8):
    """launches of the decode_sample family in one step of a HostModel / HostBatch (0: the step is the greedy graph)"""
    d = Dec.__new__(Dec)
    d.o = o
    return d.sampler_launches(n)


def test_serve_records_equal_generation_alone(hip):
    """28 prompts through 4 and 16 slots with 8-step slices and 20 new ids at most (uneven lengths: slots repeat their last step
    inside a slice and are reused): every prompt's ids and records equal the same prompt generated alone at the same width; a prompt
    that did not ask gets zeros, nothing of the slot's previous tenant; the ids are serve_biased's"""
    host = load_package().load_host()
    cfg, weights = model_setup(host, max_ctx=96, seed=1618)
    V = cfg.n_vocab
    n = 28
    lengths = [3 + (11 * j) % 40 for j in range(n)]
    prompts = [list(host.synthetic_tokens(L, seed=500 + j, n_vocab=V)) for j, L in enumerate(lengths)]
    total, seed, temp = 90, 13, 0.9
    max_new_each = [5 + (7 * j) % 16 for j in range(n)]
    ks = [0 if j % 3 == 1 else 40 for j in range(n)]
    tables = [(-1, 1)[(j // 2) % 2] for j in range(n)]
    tops = [(-1, 0, 3, 20, 5)[j % 5] for j in range(n)]
    allow = sorted(np.random.default_rng(9).choice(V, 32, replace=False).tolist())
    for n_seq in (4, 16):
        want = []
        if n_seq == 4:
            m = host.model(cfg)
            for i, w in enumerate(weights):
                m.set_weight(i, w)
            m.set_bias_table(1, allow=allow)
            for j, p in enumerate(prompts):
                ids, lp, ti, tl = m.generate_logprobs(p, len(p) + max_new_each[j], max(tops[j], 0), -1, ks[j], temp, seed, j, tables[j], 0)
                want.append((ids, lp, ti, tl))
            m.close()
        b = host.batch(cfg, n_seq)
        for i, w in enumerate(weights):
            b.set_weight(i, w)
        b.set_bias_table(1, allow=allow)
        if n_seq == 16:
            # (the wide step forms are not bit-equal to the single-sequence decoder, DESIGN 3.4: "alone" is the same decoder outside any queue)
            for lo in range(0, n, 16):
                js = [min(j, n - 1) for j in range(lo, lo + 16)]
                ids, lp, ti, tl = b.generate_logprobs([prompts[j] for j in js], total, [max(tops[j], 0) for j in js], -1, [ks[j] for j in js], temp, seed,
                                                      js, [tables[j] for j in js], None)
                for i, j in enumerate(js[: min(16, n - lo)]):
                    end = len(prompts[j]) + max_new_each[j]
                    want.append((ids[i][:end], lp[i][:end], ti[i][:end, : max(tops[j], 0)], tl[i][:end, : max(tops[j], 0)]))
        plain, _ = b.serve_biased(prompts, total, -1, ks, temp, seed, tables, None, slice_steps=8, max_new_each=max_new_each)
        for sched in (1, 3):
            b.set_serve_schedule(sched)
            got, st, lp, ti, tl = b.serve_logprobs(prompts, total, -1, ks, temp, seed, tops, tables, None, slice_steps=8, max_new_each=max_new_each)
            assert st["admissions"] == n
            for j in range(n):
                L = len(got[j])
                assert got[j].tolist() == plain[j].tolist() == want[j][0].tolist(), (n_seq, sched, j)
                assert not lp[j][: lengths[j]].any() and not lp[j][L:].any() and (ti[j][: lengths[j]] == -1).all() and (ti[j][L:] == -1).all()
                if tops[j] < 0:
                    assert not lp[j].any() and (ti[j] == -1).all() and not tl[j].any(), (n_seq, sched, j)
                    continue
                t = tops[j]
                assert (bits(lp[j][:L]) == bits(want[j][1])).all(), (n_seq, sched, j)
                assert ti[j][:L, :t].tolist() == want[j][2].tolist() and (bits(tl[j][:L, :t]) == bits(want[j][3])).all(), (n_seq, sched, j)
                assert (ti[j][:, t:] == -1).all() and not tl[j][:, t:].any()
                assert (lp[j][lengths[j]:L] <= 0).all() and lp[j][lengths[j]:L].any()
            # every slot's request was cleared when the queue was done: the step is the greedy graph again
            assert sampler_launches(b) == 0
        b.set_serve_schedule(0)
        b.close()


# ---------------------------------------------------------------------------------------------------------------- the rest

def test_score_with_alternatives_equals_the_operator_on_logits_all(hip):
    host = load_package().load_host()
    cfg, weights = model_setup(host)
    V = cfg.n_vocab
    m = host.model(cfg)
    for i, w in enumerate(weights):
        m.set_weight(i, w)
    text = host.synthetic_tokens(40, seed=77, n_vocab=V)
    for start in (0, 7):
        lp, rk = m.score(text, start)
        lp3, rk3, ti, tl = m.score(text, start, n_top=3)
        assert (bits(lp3) == bits(lp)).all() and rk3.tolist() == rk.tolist()
        rows = m.logits_all(text, start)
        targets = np.append(text[start + 1:], -1).astype(np.int32)
        olp, oti, otl = hip.row_top_logprobs(upload(hip, rows)[0], len(rows), V, V, targets, 3)
        assert ti.tolist() == oti.tolist() and (bits(tl) == bits(otl)).all()
        assert close(lp, olp)
        for r in range(len(rows)):
            assert (rk[r] < 3) == (targets[r] in ti[r].tolist()) or targets[r] < 0
    m.close()


def test_cli_logprobs_lines_match_generate_logprobs(hip, tmp_path):
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
    want_greedy = m.generate_logprobs(prompt, n_pred, 2, 32002, 0, 1.0, 0, 0, -1, 0)
    want_topk = m.generate_logprobs(prompt, n_pred, 2, 32002, 40, 0.9, 7, 0, 0, 6)
    m.close()
    for extra, (ids, lp, ti, tl) in ((["-greedy"], want_greedy), (["--seed", "7", "--topk", "40", "--temp", "0.9", "--ban", "200", "--min-new", "6"], want_topk)):
        r = subprocess.run([pkg.build.HOST_CLI, "-q4", "--ids", "--npred", str(n_pred), "--model", ckpt, "--tokenizer", vocab, "-p", "hello world",
                            "--logprobs", "2"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.strip().split("\n")
        new = ids[len(prompt):]
        assert [int(v) for v in lines[0].split()] == new.tolist()
        recs = lines[1:]
        assert len(recs) == len(new)
        for i, line in enumerate(recs):
            f = line.split()
            pos = len(prompt) + i
            assert len(f) == 4 and int(f[0]) == new[i] and np.float32(f[1]) == lp[pos], (i, line, lp[pos])
            for a in range(2):
                tid, tlp = f[2 + a].split(":")
                assert int(tid) == ti[pos][a] and np.float32(tlp) == tl[pos][a], (i, line)
