"""-m gpu: scoring given ids (include/gten_hip_score.h, include/gten_host_score.h).

1. gten_hip_row_logprobs against numpy float64: widths 32003 / 32000 / 4099 / 65 / 1, padded (16-byte rows) and odd strides,
   ties at the maximum and at the target, a +-80 spread, unscored rows; rank and argmax exact.
2. score / logits_all of a tiny model against the oracle's logits(tokens[:t + 1], 0): the logits in the golden band, the
   log-prob within the Lipschitz bound of log-softmax (2 max|d logit| + 1e-4), the rank wherever the oracle's gap allows.
3. score against float64 log-softmax of logits_all on the same ids.
4. the K / V caches after score: the next fused decode row is the bytes it is after logits().
5. score_many: a text's bytes do not depend on its group; short texts go one by one; near score on the same text.
6. bad arguments return < 0.
"""
import numpy as np
import pytest

from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from helpers import MODES, Q4, Q8, tiny_config

pytestmark = pytest.mark.gpu


def ref_logprobs(x, t):
    """float64 log-softmax at t, rank under (x > x_t) or (x == x_t and j < t), first maximum"""
    x64 = x.astype(np.float64)
    m = x64.max()
    lp = x64[t] - (m + np.log(np.exp(x64 - m).sum()))
    rank = int((x > x[t]).sum() + (x[:t] == x[t]).sum())
    return lp, rank, int(np.argmax(x))


def pad4(v):
    return (v + 3) // 4 * 4


@pytest.mark.parametrize("V", [32003, 32000, 4099, 65, 1])
def test_row_logprobs_against_numpy(hip, V):
    r = np.random.default_rng(V)
    n_rows = 300
    for stride in (pad4(V), V | 1):
        x = (r.standard_normal((n_rows, V)) * 3).astype(np.float32)
        x[1::3] = np.round(x[1::3] * 2) / 2                     # many ties
        t = r.integers(0, V, n_rows).astype(np.int32)
        if V >= 4:
            x[0, :] = -1.0; x[0, 2] = 5.0; x[0, V - 1] = 5.0; t[0] = V - 1            # the maximum twice, target the second
            x[1, :] = 0.0; x[1, 1] = 1.0; x[1, V // 2] = 1.0; x[1, V - 1] = 1.0; t[1] = V // 2   # tied before and after
            x[2] = r.uniform(-80, 80, V).astype(np.float32); x[2, 0] = 80.0; t[2] = V - 1; x[2, V - 1] = -80.0
            x[3] = np.float32(80.0) * np.sign(r.standard_normal(V)).astype(np.float32); t[3] = 1
        t[5::7] = -1
        buf = np.zeros((n_rows, stride), np.float32)
        buf[:, :V] = x
        dev = hip.upload(buf)
        lp, rank, am = hip.row_logprobs(dev, n_rows, V, stride, t)
        for i in range(n_rows):
            want_am = int(np.argmax(x[i]))
            assert am[i] == want_am, (V, stride, i)
            if t[i] < 0:
                assert lp[i] == 0.0 and rank[i] == -1, (V, stride, i)
                continue
            wlp, wrank, _ = ref_logprobs(x[i], int(t[i]))
            assert abs(lp[i] - wlp) <= 1e-4 + 1e-6 * abs(wlp), (V, stride, i, lp[i], wlp)
            assert rank[i] == wrank, (V, stride, i, rank[i], wrank)
        for i in range(12):                                       # the greedy rule of gten_hip_argmax_row
            assert am[i] == hip.argmax_row(dev, V, offset=4 * i * stride), (V, stride, i)
        # without rank / argmax outputs: the log-probs alone, same values
        assert hip.row_logprobs_rc(dev, n_rows, V, stride) == 0


def test_row_logprobs_bad_arguments(hip):
    dev = hip.upload(np.zeros((4, 8), np.float32))
    assert hip.row_logprobs_rc(dev, 4, 0, 8) != 0                # n_vocab < 1
    assert hip.row_logprobs_rc(dev, 4, 9, 8) != 0                # row_stride < n_vocab
    assert hip.row_logprobs_rc(dev, 0, 8, 8) != 0
    assert hip.row_logprobs_rc(dev, 65536, 8, 8) != 0


def host_cfg(c):
    pkg = load_package()
    return pkg.HostConfig(**{k: getattr(c, k) for k, _ in c._fields_})


def lipschitz_check(lp, rank, lg_gpu, lg_ref, t):
    """|d logprob| <= 2 max|d logit| + 1e-4; the rank where the reference's gap around the target exceeds 2 max|d logit|"""
    dmax = float(np.abs(lg_gpu.astype(np.float64) - lg_ref).max())
    wlp, wrank, _ = ref_logprobs(lg_ref.astype(np.float32), t)
    assert abs(float(lp) - wlp) <= 2 * dmax + 1e-4, (lp, wlp, dmax)
    x = lg_ref.astype(np.float64)
    others = np.delete(x, t) - x[t]
    if others.size and np.abs(others).min() > 2 * dmax:
        assert rank == wrank, (rank, wrank, dmax)


# every mode; the quantized ones in both prefill forms (fast and exact, gten_hip_set_prefill_exact)
FORMS = [(name, wd, ad, exact) for name, wd, ad in MODES() for exact in ((False,) if name == "f16" else (False, True))]


@pytest.mark.parametrize("name,wd,ad,exact", FORMS)
def test_tiny_model_score_against_oracle(hip, oracle, name, wd, ad, exact):
    from test_golden_gpu import band
    pkg = load_package()
    host = pkg.load_host()
    ocfg = tiny_config(wd, ad, n_heads=4, n_kv_heads=2, max_ctx=512)
    cfg = host_cfg(ocfg)
    gm, om = host.model(cfg), oracle.model(ocfg)
    for i in range(gm.n_weights()):
        w = host.synth_weight(cfg, 9100, i)
        gm.set_weight(i, w); om.set_weight(i, w)
    hip.set_prefill_exact(exact)
    try:
        for n in (17, 100, 300):
            toks = host.synthetic_tokens(n, seed=n, n_vocab=cfg.n_vocab)
            all_lg = gm.logits_all(toks, 0)
            lp, rank = gm.score(toks, 0)
            assert all_lg.shape == (n, cfg.n_vocab) and lp[-1] == 0 and rank[-1] == -1
            for t in sorted(set(np.linspace(0, n - 2, 8).astype(int).tolist()) | {0, n - 2}):
                want = np.asarray(om.logits(list(toks[: t + 1]), 0), np.float64)
                band(name, all_lg[t] - want, float(want.std()))
                lipschitz_check(lp[t], rank[t], all_lg[t], want, int(toks[t + 1]))
            # the last row as well (it has no target by default)
            want = np.asarray(om.logits(list(toks), 0), np.float64)
            band(name, all_lg[n - 1] - want, float(want.std()))
        # start_pos > 0: the prefix through logits(), then score of the rest
        toks = host.synthetic_tokens(120, seed=5, n_vocab=cfg.n_vocab)
        s = 70
        gm.logits(toks[:s], 0)
        lp, rank = gm.score(toks, s)
        assert len(lp) == 120 - s
        for t in (s, s + 1, 100, 118):
            want = np.asarray(om.logits(list(toks[: t + 1]), 0), np.float64)
            gm.logits(toks[:s], 0)
            row = gm.logits_all(toks[: t + 1], s)[-1]
            band(name, row - want, float(want.std()))
            lipschitz_check(lp[t - s], rank[t - s], row, want, int(toks[t + 1]))
    finally:
        hip.set_prefill_exact(False)
    gm.close(); om.close()


@pytest.mark.parametrize("name,wd,ad", MODES())
def test_score_is_log_softmax_of_logits_all(hip, name, wd, ad):
    pkg = load_package()
    host = pkg.load_host()
    cfg = host_cfg(tiny_config(wd, ad, n_heads=4, n_kv_heads=2, max_ctx=1024))
    gm = host.model(cfg)
    gm.load_synthetic(31)
    for n, sp in ((700, 0), (40, 0), (8, 0), (700, 650), (700, 699)):
        toks = host.synthetic_tokens(n, seed=n + sp, n_vocab=cfg.n_vocab)
        if sp:
            gm.logits(toks[:sp], 0)
        lg = gm.logits_all(toks, sp)
        if sp:
            gm.logits(toks[:sp], 0)
        tg = np.random.default_rng(n).integers(0, cfg.n_vocab, n - sp).astype(np.int32)
        tg[::5] = -1
        lp, rank = gm.score(toks, sp, tg)
        for i in range(n - sp):
            if tg[i] < 0:
                assert lp[i] == 0 and rank[i] == -1
                continue
            wlp, wrank, _ = ref_logprobs(lg[i], int(tg[i]))
            assert abs(lp[i] - wlp) <= 1e-4, (n, sp, i, lp[i], wlp)
            assert rank[i] == wrank, (n, sp, i)
        greedy = np.argmax(lg, axis=1).astype(np.int32)
        lp0, rank0 = gm.score(toks, sp, greedy) if not sp else (None, None)
        if rank0 is not None:
            assert (rank0 == 0).all()
    gm.close()


@pytest.fixture(scope="module")
def full_q4(hip):
    pkg = load_package()
    host = pkg.load_host()
    m = host.model(host.default_config(Q4, Q8))
    m.load_synthetic(2024)
    yield host, m
    m.close()


def test_caches_after_score_continue_like_logits(full_q4):
    host, m = full_q4
    P = host.synthetic_tokens(300, seed=3, n_vocab=32003)
    x = 1234
    nxt = np.append(P, x).astype(np.int32)
    wants = []
    for sp in (0, len(P) - 1):
        if sp:
            m.logits(P[:sp], 0)
        m.logits(P, sp)
        want = m.logits(nxt, len(P))
        wants.append(want)
        if sp:
            m.logits(P[:sp], 0)
        m.score(P, sp)
        got = m.logits(nxt, len(P))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), sp
    # one new row: the fused decoder's logits buffer is the row that gets scored
    want = wants[0]
    m.logits(P, 0)
    lp, rank = m.score(nxt, len(P), [int(np.argmax(want))])
    assert rank[0] == 0
    wlp, _, _ = ref_logprobs(want, int(np.argmax(want)))
    assert abs(lp[0] - wlp) <= 1e-4


def test_score_many_groups(full_q4):
    host, m = full_q4
    r = np.random.default_rng(7)
    texts = [host.synthetic_tokens(int(n), seed=100 + i, n_vocab=32003) for i, n in enumerate(r.integers(16, 240, 40))]
    texts[5] = host.synthetic_tokens(300, seed=99, n_vocab=32003)
    assert sum(len(t) for t in texts) > 4096
    tgt = texts[5]
    lp_alone, rk_alone = m.score_many([tgt])
    lp_three, rk_three = m.score_many([texts[0], tgt, texts[1]])
    lp_all, rk_all = m.score_many(texts)
    for lp, rk in ((lp_three[1], rk_three[1]), (lp_all[5], rk_all[5])):
        assert np.array_equal(lp.view(np.uint32), lp_alone[0].view(np.uint32))
        assert np.array_equal(rk, rk_alone[0])
    # a short text (one by one) beside grouped ones: what score gives it
    short = host.synthetic_tokens(9, seed=1, n_vocab=32003)
    lp_mix, rk_mix = m.score_many([texts[0], short, tgt])
    lp_s, rk_s = m.score(short, 0)
    assert np.array_equal(lp_mix[1].view(np.uint32), lp_s.view(np.uint32)) and np.array_equal(rk_mix[1], rk_s)
    assert np.array_equal(lp_mix[2].view(np.uint32), lp_alone[0].view(np.uint32))
    # near score on the same text: within the Lipschitz bound of the logit band
    lp_one, _ = m.score(tgt, 0)
    lg = m.logits_all(tgt, 0)
    s = max(float(lg.std()) / 0.91, 1.0)
    assert np.abs(lp_one - lp_alone[0]).max() <= 2 * 0.5 * s + 1e-4
    assert lp_alone[0][-1] == 0 and rk_alone[0][-1] == -1


def test_bad_arguments(full_q4):
    host, m = full_q4
    toks = host.synthetic_tokens(20, seed=2, n_vocab=32003)
    assert m.score_rc(toks, 0, np.full(20, 32003, np.int32))[0] < 0          # a target >= n_vocab
    assert m.score_rc(toks, 0, np.full(20, -2, np.int32))[0] < 0
    assert m.score_rc(toks, 20)[0] < 0                                         # n - start_pos < 1
    assert m.score_rc(host.synthetic_tokens(2049, seed=2, n_vocab=32003), 0)[0] < 0
    assert m.score_many_rc([toks, host.synthetic_tokens(2049, seed=3, n_vocab=32003)])[0] < 0   # a text over 2048 ids
    assert m.score_many_rc([toks, toks[:0]])[0] < 0                            # an empty text
    assert m.score_many_rc([toks], [np.full(20, 40000, np.int32)])[0] < 0
    lp, rank = m.score(toks, 0)                                                # and the model still scores afterwards
    assert np.isfinite(lp).all() and rank[-1] == -1
