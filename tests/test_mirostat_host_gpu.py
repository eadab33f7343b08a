"""-m gpu: generation under Mirostat v2 through the host flows and the command line (include/gten_host_mirostat.h).

Ten prompts at 2048 ids, each alone on a model, the first four as a batch of four, and all of them as a queue through four slots under
two schedules: the same ids per prompt -- mu travels with the prompt, whatever slot takes it.  No binding is left behind, also after
refused calls.  The command line's ids are generate_mirostat's."""
import subprocess

import numpy as np
import pytest

from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from test_bias_gpu import NINF
from test_nucleus_gpu import model_setup

pytestmark = pytest.mark.gpu


def test_generate_batch_and_serve_agree_and_leave_no_binding(hip):
    pkg = load_package()
    host = pkg.load_host()
    cfg, weights = model_setup(host, 2048, max_ctx=96, seed=1618)          # (2048 ids: the whole-vocabulary prompts take the row-wide routine)
    V = cfg.n_vocab
    n, n_seq = 10, 4
    lengths = [3 + (11 * j) % 40 for j in range(n)]
    prompts = [list(host.synthetic_tokens(L, seed=500 + j, n_vocab=V)) for j, L in enumerate(lengths)]
    total, seed, temp = 90, 13, 0.9
    max_new_each = [5 + (7 * j) % 16 for j in range(n)]
    ks = [0 if j % 5 == 4 else V if j % 5 == 3 else 40 for j in range(n)]                        # greedy, whole-vocabulary and top-k 40 prompts
    taus = [(3.0, 5.0, 0.0, 2.0, 4.0)[j % 5] for j in range(n)]                                  # (tau 0: this prompt is not under Mirostat)
    etas = [(0.1, 0.25, 0.1, 1.0, 0.1)[j % 5] for j in range(n)]
    tables = [(-1, 1)[(j // 2) % 2] for j in range(n)]
    reps = [(1.0, 1.3)[(j // 3) % 2] for j in range(n)]
    allow = sorted(np.random.default_rng(9).choice(V, 64, replace=False).tolist())
    m = host.model(cfg)
    for i, w in enumerate(weights):
        m.set_weight(i, w)
    m.set_bias_table(1, allow=allow)
    alone, plain = [], []
    for j, p in enumerate(prompts):
        L = len(p) + max_new_each[j]
        alone.append(m.generate_mirostat(p, L, taus[j], etas[j], -1, ks[j], temp, seed, j, rep=reps[j], table=tables[j]))
        plain.append(m.generate_mirostat(p, L, 0.0, 0.1, -1, ks[j], temp, seed, j, rep=reps[j], table=tables[j]))
        want = m.generate_penalized(p, L, -1, ks[j], temp, seed, j, reps[j], table=tables[j])
        assert plain[j].tolist() == want.tolist(), j                                             # tau 0: the flow below, id for id
        if ks[j] == 0 or taus[j] == 0.0:
            assert alone[j].tolist() == plain[j].tolist(), j                                     # a greedy prompt ignores Mirostat
    assert not m.mirostat_info()[0].any() and m.mirostat_info()[3]
    assert sum(a.tolist() != p.tolist() for a, p in zip(alone, plain)) >= 3                      # Mirostat changed something
    # refused calls leave no binding: a cut beside Mirostat (by name), a tau and an eta outside their ranges
    for kw in (dict(top_p=0.9), dict(min_p=0.1)):
        with pytest.raises(pkg.GtenHipError):
            m.generate_mirostat(prompts[0], 40, 3.0, 0.1, -1, 40, temp, seed, 0, **kw)
    for tau, eta in ((40.0, 0.1), (-1.0, 0.1), (3.0, 0.0), (3.0, 1.5), (float("nan"), 0.1)):
        with pytest.raises(pkg.GtenHipError):
            m.generate_mirostat(prompts[0], 40, tau, eta, -1, 40, temp, seed, 0)
    assert m.generate_mirostat(prompts[0], 40, 3.0, 0.1, -1, 0, temp, seed, 0, top_p=0.9).tolist() == m.generate(prompts[0], 40).tolist()   # (greedy: neither acts)
    assert not m.mirostat_info()[0].any() and m.cut_info()[:2] == (1.0, 0.0)
    m.close()
    b = host.batch(cfg, n_seq)
    for i, w in enumerate(weights):
        b.set_weight(i, w)
    b.set_bias_table(1, allow=allow)
    first = list(range(n_seq))
    ids = b.generate_mirostat([prompts[j] for j in first], total, [taus[j] for j in first], [etas[j] for j in first], -1, [ks[j] for j in first], temp, seed,
                              first, rep=[reps[j] for j in first], tables=[tables[j] for j in first])
    for j in first:
        L = len(alone[j])
        assert ids[j][:L].tolist() == alone[j].tolist(), j
    assert not b.mirostat_info()[0].any() and b.mirostat_info()[3]
    for sched in (1, 3):
        b.set_serve_schedule(sched)
        got, st = b.serve_mirostat(prompts, total, -1, ks, temp, seed, taus, etas, rep=reps, tables=tables, slice_steps=8, max_new_each=max_new_each)
        assert st["admissions"] == n
        for j in range(n):
            assert got[j].tolist() == alone[j].tolist(), (sched, j)
        assert not b.mirostat_info()[0].any()
    b.set_serve_schedule(0)
    with pytest.raises(pkg.GtenHipError):
        b.generate_mirostat([prompts[j] for j in first], total, [3.0, 3.0, 0.0, 3.0], 0.1, -1, 40, temp, seed, first, top_p=[1.0, 1.0, 0.9, 0.9])
    with pytest.raises(pkg.GtenHipError):
        b.serve_mirostat(prompts, total, -1, 40, temp, seed, 3.0, 0.1, min_p=0.2)
    with pytest.raises(pkg.GtenHipError):
        b.serve_mirostat(prompts, total, -1, 40, temp, seed, 33.0, 0.1)
    assert not b.mirostat_info()[0].any()
    a, c, _, _ = b.cut_info()
    assert (a == 1.0).all() and (c == 0.0).all()
    # a cut on an item that is NOT under Mirostat, beside items that are, is served
    got, _ = b.serve_mirostat(prompts[:4], total, -1, 40, temp, seed, [3.0, 0.0, 3.0, 0.0], 0.1, top_p=[1.0, 0.9, 1.0, 0.5], slice_steps=8, max_new=6)
    assert all(len(g) == len(p) + 6 for g, p in zip(got, prompts[:4]))
    b.close()


def test_cli_mirostat_prints_the_ids_of_generate_mirostat(hip, tmp_path):
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
    want = m.generate_mirostat(prompt, n_pred, 5.0, 0.1, 32002, 40, 0.9, 7, 0)
    want_all = m.generate_mirostat(prompt, n_pred, 3.0, 0.5, 32002, 32003, 0.9, 7, 0, table=0)
    m.close()
    assert want.tolist() != plain.tolist() or want_all.tolist() != plain.tolist()
    common = [pkg.build.HOST_CLI, "-q4", "--ids", "--npred", str(n_pred), "--model", ckpt, "--tokenizer", vocab, "-p", "hello world", "--seed", "7", "--temp", "0.9"]
    r = subprocess.run(common + ["--topk", "40", "--mirostat", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [int(v) for v in r.stdout.split()] == want[len(prompt):].tolist()
    r = subprocess.run(common + ["--topk", "32003", "--mirostat", "2", "--mirostat-ent", "3", "--mirostat-lr", "0.5", "--ban", "200"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [int(v) for v in r.stdout.split()] == want_all[len(prompt):].tolist()
    r = subprocess.run(common + ["--topk", "40", "--mirostat", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and [int(v) for v in r.stdout.split()] == plain[len(prompt):].tolist()


def test_mu_moves_with_a_prompt_between_lanes_in_the_tail(hip):
    """a queue through 256 slots (two lanes) under the free schedule: in the tail the sequences of the emptier lane move to the other, and
    the mu a moved prompt's next id is drawn under is read back and goes with it -- the ids are those of the same queue through 16 slots,
    where nothing moves"""
    from helpers import Q4, Q8, tiny_config
    from test_model_gpu import host_cfg
    from test_serving_gpu import make_prompts
    host = load_package().load_host()
    cfg = host_cfg(tiny_config(Q4, Q8, n_heads=4, n_kv_heads=2, max_ctx=128, n_layers=2))
    weights = [host.synth_weight(cfg, 1414, i) for i in range(len(cfg.weight_shapes()))]
    n = 140
    prompts = make_prompts(host, cfg, [8 + (23 * i) % 63 for i in range(n)], 17)
    budgets = np.array([4 + (11 * i) % 31 for i in range(n)], np.int32)
    ks = [0 if j % 3 == 2 else 40 for j in range(n)]
    taus = [0.0 if j % 4 == 3 else 3.0 for j in range(n)]
    outs, stats = [], []
    for slots in (256, 16):
        b = host.batch(cfg, slots)
        for i, w in enumerate(weights):
            b.set_weight(i, w)
        got, st = b.serve_mirostat(prompts, 128, -1, ks, 0.9, 13, taus, 0.25, slice_steps=8, max_new_each=budgets)
        assert st["admissions"] == n and not b.mirostat_info()[0].any()
        outs.append(got); stats.append(st)
        b.close()
    print("moved:", stats[0]["moved"], stats[1]["moved"])
    assert stats[0]["moved"] > 0 and stats[1]["moved"] == 0
    for j in range(n):
        assert len(outs[0][j]) == len(prompts[j]) + budgets[j] and outs[0][j].tolist() == outs[1][j].tolist(), j
