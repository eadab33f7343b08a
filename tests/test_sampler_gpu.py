"""-m gpu: top-k sampling with a temperature on the device (include/gten_hip_sample.h, csrc/gten_decode_sample.h).

The ids are held to tests/sample_ref.py, the contract restated in numpy: exactly on the candidate set (integer
arithmetic), and on the draw except where two candidates' scores lie within f32 rounding of each other (the device
scores in f32, the restatement in float64) -- such a near tie must be within 1e-4 and at most 0.1 % of draws may need it."""
import numpy as np
import pytest

import sample_ref as ref
from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from helpers import MODES, Q4, Q8, tiny_config
from test_model_gpu import host_cfg

pytestmark = pytest.mark.gpu

NEAR = 1e-4


def upload_rows(hip, rows):
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    return load_package().hipabi.DeviceBuffer.from_numpy(hip, rows)


def crafted_rows(n_vocab, n_rows, seed):
    """logits with many exact ties (values on a grid of 1/8) and a few rows of one repeated value"""
    r = np.random.default_rng(seed)
    x = np.round(r.standard_normal((n_rows, n_vocab)) * 16.0) / 8.0
    x[0, :] = 0.5                                     # every value tied
    x[1, :] = -3.0
    x[1, n_vocab // 2:] = 1.25                        # the upper half tied at the top
    return x.astype(np.float32)


def check_draws(rows, ids, top_k, temp, seed, streams, positions):
    """every id is a candidate; ids equal the restatement but for near ties; returns the number of excused draws"""
    excused = 0
    for r in range(len(ids)):
        x = rows[r if rows.shape[0] > 1 else 0]
        k, t, s, p = int(top_k[r]), float(temp[r]), int(streams[r]), int(positions[r])
        got = int(ids[r])
        if k == 0:
            assert got == int(np.argmax(x)), r
            continue
        assert got in set(ref.candidates(x, k).tolist()), (r, got, k)
        want, _ = ref.draw(x, k, t, seed, s, p)
        if got != want:
            gap = ref.score_of(x, want, t, seed, s, p) - ref.score_of(x, got, t, seed, s, p)
            assert 0.0 <= gap <= NEAR, (r, got, want, gap)
            excused += 1
    return excused


@pytest.mark.parametrize("n_vocab", [512, 32003, 65535])
def test_operator_draws_follow_the_contract(hip, n_vocab):
    n_rows = 96 if n_vocab > 1000 else 512
    rows = crafted_rows(n_vocab, n_rows, 11 + n_vocab)
    buf = upload_rows(hip, rows)
    r = np.random.default_rng(n_vocab)
    ks = np.array([1, 2, 3, 5, 40, 50, 1000, n_vocab - 1, n_vocab, n_vocab + 7, 0])
    top_k = ks[np.arange(n_rows) % len(ks)].astype(np.int32)
    temp = r.choice([0.25, 0.9, 1.0, 3.0], n_rows).astype(np.float32)
    streams = r.integers(0, 1 << 32, n_rows, dtype=np.uint64).astype(np.uint32)
    positions = r.integers(1, 1 << 20, n_rows).astype(np.int32)
    seed = 0x1234_5678_9ABC_DEF0
    ids = hip.sample_rows(buf, n_rows, n_vocab, n_vocab, top_k, temp, seed, streams, positions)
    excused = check_draws(rows, ids, top_k, temp, seed, streams, positions)
    assert excused <= max(1, n_rows // 1000), excused
    # ties at the threshold go to the lower index: every value tied -> the first k indices only
    for k in (1, 3, 40):
        got = hip.sample_rows(buf, 64, n_vocab, 0, k, 1.0, 5, np.arange(64), 9)
        assert (got < k).all() and (got >= 0).all(), got
        if k == 40:
            assert len(set(got.tolist())) > 10                     # ... and the draw spreads over them
    # row 1: the upper half is tied at the top; k below its size takes its first k indices
    got = hip.sample_rows(upload_rows(hip, rows[1:2]), 64, n_vocab, 0, 7, 2.0, 5, np.arange(64), 3)
    assert ((got >= n_vocab // 2) & (got < n_vocab // 2 + 7)).all(), got


def test_operator_argument_errors(hip):
    buf = upload_rows(hip, np.zeros((1, 16), np.float32))
    assert hip.sample_rows_rc(buf, 1, 16, 16, 5, 0.0) != 0              # temp 0 with top_k >= 1
    assert hip.sample_rows_rc(buf, 1, 16, 16, 5, float("nan")) != 0
    assert hip.sample_rows_rc(buf, 1, 16, 16, 5, float("inf")) != 0
    assert hip.sample_rows_rc(buf, 1, 16, 16, -1, 1.0) != 0
    assert hip.sample_rows_rc(buf, 1, 0, 16, 5, 1.0) != 0                # n_vocab outside [1, 65535]
    assert hip.sample_rows_rc(buf, 1, 65536, 16, 5, 1.0) != 0
    assert hip.sample_rows_rc(buf, 1, 16, 16, 0, 0.0) == 0               # greedy: the temperature is not looked at
    assert hip.sample_rows_rc(buf, 1, 16, 16, 3, 0.5) == 0


def test_draws_follow_top_k_softmax(hip):
    """2^18 draws from one row (k 40, T 0.9; positions and streams varied): chi^2 against the exact top-k softmax below
    96.1, the 1e-6 upper quantile at 39 degrees of freedom (fixed seeds: deterministic)"""
    n, k, temp = 512, 40, 0.9
    r = np.random.default_rng(3)
    x = (-0.05 * r.permutation(n)).astype(np.float32)               # distinct values, the top 40 within a factor of ~9
    buf = upload_rows(hip, x[None, :])
    N = 1 << 18
    pos = (np.arange(N) % 4096 + 1).astype(np.int32)
    streams = (np.arange(N) // 4096).astype(np.uint32)
    ids = hip.sample_rows(buf, N, n, 0, k, temp, 0xC0FFEE, streams, pos)
    c = ref.candidates(x, k)
    assert np.isin(ids, c).all()
    z = x[c].astype(np.float64) / temp
    p = np.exp(z - z.max())
    p /= p.sum()
    obs = np.array([(ids == j).sum() for j in c], np.float64)
    chi2 = float((((obs - N * p) ** 2) / (N * p)).sum())
    assert chi2 < 96.1, chi2


def tiny_model(host, wd, ad, seed=4242, **kw):
    cfg = host_cfg(tiny_config(wd, ad, **kw))
    m = host.model(cfg)
    for i in range(len(cfg.weight_shapes())):
        m.set_weight(i, host.synth_weight(cfg, seed, i))
    return cfg, m


@pytest.mark.parametrize("name,wd,ad", MODES())
def test_decoder_draws_follow_the_contract(hip, name, wd, ad):
    """sampled generation, replayed teacher-forced: every step's logits give the restatement's id (near ties excused)"""
    host = load_package().load_host()
    cfg, m = tiny_model(host, wd, ad, max_ctx=160)
    prompt = list(host.synthetic_tokens(9, seed=77, n_vocab=cfg.n_vocab))
    seed, stream, k, temp = 99, 3, 40, 0.9
    ids = m.generate_topk(prompt, 150, -1, k, temp, seed, stream)
    assert len(ids) == 150 and ids[:9].tolist() == prompt
    excused = 0
    for p in range(len(prompt), len(ids)):
        x = m.logits(ids[:p], 0 if p == len(prompt) else p - 1)
        got = int(ids[p])
        assert got in set(ref.candidates(x, k).tolist()), p
        want, _ = ref.draw(x, k, temp, seed, stream, p)
        if got != want:
            gap = ref.score_of(x, want, temp, seed, stream, p) - ref.score_of(x, got, temp, seed, stream, p)
            assert 0.0 <= gap <= NEAR, (p, got, want, gap)
            excused += 1
    assert excused <= 1
    greedy = m.generate(prompt, 150)
    assert ids.tolist() != greedy.tolist()                          # (the draw is not the argmax)
    m.close()


@pytest.mark.parametrize("n_seq", [1, 8, 64, 256])
def test_top_k_one_and_zero_are_greedy(hip, n_seq):
    host = load_package().load_host()
    cfg = host_cfg(tiny_config(Q4, Q8, n_heads=4, n_kv_heads=2, max_ctx=96))
    weights = [host.synth_weight(cfg, 555, i) for i in range(len(cfg.weight_shapes()))]
    lengths = [3 + (7 * i) % 40 for i in range(n_seq)]
    prompts = [list(host.synthetic_tokens(n, seed=300 + i, n_vocab=cfg.n_vocab)) for i, n in enumerate(lengths)]
    total = 80
    if n_seq == 1:
        m = host.model(cfg)
        for i, w in enumerate(weights):
            m.set_weight(i, w)
        want = m.generate(prompts[0], total)
        for k, t in ((1, 0.3), (1, 5.0), (0, 1.0)):
            assert m.generate_topk(prompts[0], total, -1, k, t, 17).tolist() == want.tolist(), (k, t)
        assert m.generate(prompts[0], total).tolist() == want.tolist()       # the decoder is greedy again afterwards
        m.close()
        return
    b = host.batch(cfg, n_seq)
    for i, w in enumerate(weights):
        b.set_weight(i, w)
    want = b.generate(prompts, total)
    for k, t in ((1, 0.3), (0, 1.0)):
        got = b.generate_topk(prompts, total, -1, k, t, 17)
        for q in range(n_seq):
            assert got[q].tolist() == want[q].tolist(), (k, q)
    again = b.generate(prompts, total)
    assert all(a.tolist() == w.tolist() for a, w in zip(again, want))
    b.close()


@pytest.mark.parametrize("name,wd,ad", MODES())
def test_batch_width_and_seed(hip, name, wd, ad):
    """sampled batch generation at 2 and 8 sequences equals the single-sequence decoder with the same stream; one seed
    repeats, another seed differs"""
    host = load_package().load_host()
    cfg = host_cfg(tiny_config(wd, ad, n_heads=4, n_kv_heads=2, max_ctx=128))      # (several sequences: 64-wide heads)
    weights = [host.synth_weight(cfg, 808, i) for i in range(len(cfg.weight_shapes()))]
    prompts = [list(host.synthetic_tokens(4 + 5 * i, seed=40 + i, n_vocab=cfg.n_vocab)) for i in range(8)]
    streams = [7 * q + 1 for q in range(8)]
    total, k, temp, seed = 100, 40, 0.9, 2024
    m = host.model(cfg)
    for i, w in enumerate(weights):
        m.set_weight(i, w)
    alone = [m.generate_topk(p, total, -1, k, temp, seed, s) for p, s in zip(prompts, streams)]
    assert m.generate_topk(prompts[0], total, -1, k, temp, seed, streams[0]).tolist() == alone[0].tolist()
    assert m.generate_topk(prompts[0], total, -1, k, temp, seed + 1, streams[0]).tolist() != alone[0].tolist()
    m.close()
    for n_seq in (2, 8):
        b = host.batch(cfg, n_seq)
        for i, w in enumerate(weights):
            b.set_weight(i, w)
        got = b.generate_topk(prompts[:n_seq], total, -1, k, temp, seed, streams[:n_seq])
        for q in range(n_seq):
            assert got[q].tolist() == alone[q].tolist(), (n_seq, q)
        b.close()


def serve_setup(host, wd, ad, n_seq, seed=31337, max_ctx=160):
    cfg = host_cfg(tiny_config(wd, ad, n_heads=4, n_kv_heads=2, max_ctx=max_ctx))
    weights = [host.synth_weight(cfg, seed, i) for i in range(len(cfg.weight_shapes()))]
    b = host.batch(cfg, n_seq)
    for i, w in enumerate(weights):
        b.set_weight(i, w)
    return cfg, weights, b


@pytest.mark.parametrize("name,wd,ad", MODES())
def test_sampled_serve_equals_generation_alone(hip, name, wd, ad):
    """a mixed queue (greedy and sampled prompts) through 2 and 8 slots: every prompt's ids are those of generating it alone
    with stream = its queue index, whatever slot it lands on and whatever the admission schedule; its greedy prompts are
    today's serve() ids; with as many prompts as slots serve equals the sampled batch.generate"""
    host = load_package().load_host()
    lengths = [5, 40, 1, 17, 90, 9, 33, 100, 2, 64, 12, 7, 21]
    cfg, weights, _ = serve_setup(host, wd, ad, 2)
    prompts = [list(host.synthetic_tokens(n, seed=900 + 3 * i, n_vocab=cfg.n_vocab)) for i, n in enumerate(lengths)]
    total, seed, temp = 150, 77, 0.9
    ks = [0 if j % 3 == 1 else 40 for j in range(len(prompts))]
    m = host.model(cfg)
    for i, w in enumerate(weights):
        m.set_weight(i, w)
    want = [m.generate(p, total) if k == 0 else m.generate_topk(p, total, -1, k, temp, seed, j) for j, (p, k) in enumerate(zip(prompts, ks))]
    eos = int(want[0][len(prompts[0]) + 20])                        # an id that comes up: some prompts stop early at it
    want_eos = [m.generate(p, total, eos) if k == 0 else m.generate_topk(p, total, eos, k, temp, seed, j)
                for j, (p, k) in enumerate(zip(prompts, ks))]
    m.close()
    for n_seq in (2, 8):
        b = host.batch(cfg, n_seq)
        for i, w in enumerate(weights):
            b.set_weight(i, w)
        got, st = b.serve_topk(prompts, total, -1, ks, temp, seed, slice_steps=16)
        assert st["admissions"] == len(prompts)
        for j in range(len(prompts)):
            assert got[j].tolist() == want[j].tolist(), (n_seq, j)
        for sched in (1, 3):
            b.set_serve_schedule(sched)
            got, _ = b.serve_topk(prompts, total, eos, ks, temp, seed, slice_steps=8)
            for j in range(len(prompts)):
                assert got[j].tolist() == want_eos[j].tolist(), (n_seq, sched, j)
        b.set_serve_schedule(0)
        greedy, _ = b.serve(prompts, total, eos, 8)
        for j in range(len(prompts)):
            if ks[j] == 0:
                assert greedy[j].tolist() == want_eos[j].tolist(), (n_seq, j)
        first = prompts[:n_seq]
        gen = b.generate_topk(first, total, -1, 40, temp, seed)
        srv, _ = b.serve_topk(first, total, -1, 40, temp, seed)
        assert all(g.tolist() == s.tolist() for g, s in zip(gen, srv)), n_seq
        b.close()


def test_sampled_serve_128_slots_equal_16_and_spares(hip):
    host = load_package().load_host()
    cfg, weights, b16 = serve_setup(host, Q4, Q8, 16, seed=2718, max_ctx=200)
    lengths = [3 + (17 * i) % 120 for i in range(160)]
    prompts = [list(host.synthetic_tokens(n, seed=50 + i, n_vocab=cfg.n_vocab)) for i, n in enumerate(lengths)]
    ks = [0 if j % 5 == 0 else 40 for j in range(len(prompts))]
    want, _ = b16.serve_topk(prompts, 180, -1, ks, 0.9, 11, max_new=30)
    b16.set_serve_spares(0)
    got, _ = b16.serve_topk(prompts, 180, -1, ks, 0.9, 11, max_new=30)
    assert all(g.tolist() == w.tolist() for g, w in zip(got, want))
    b16.close()
    b128 = host.batch(cfg, 128)
    for i, w in enumerate(weights):
        b128.set_weight(i, w)
    got, _ = b128.serve_topk(prompts, 180, -1, ks, 0.9, 11, max_new=30)
    for j in range(len(prompts)):
        assert got[j].tolist() == want[j].tolist(), j
    again, _ = b128.serve_topk(prompts, 180, -1, ks, 0.9, 11, max_new=30)
    assert all(g.tolist() == a.tolist() for g, a in zip(got, again))
    other, _ = b128.serve_topk(prompts, 180, -1, ks, 0.9, 12, max_new=30)
    assert sum(o.tolist() != g.tolist() for o, g in zip(other, got)) > len(prompts) // 2
    b128.close()


@pytest.mark.parametrize("n_seq", [64, 256])
def test_wide_sampled_ids_follow_the_sequence_not_the_slot(hip, n_seq):
    """k 40 at 64 sequences (one lane) and 256 (lanes): prompts and their streams moved to other slots give the same ids per
    prompt, so each row reads its own request (lane offsets) and its own stream; a greedy row in a sampled decoder keeps
    the argmax"""
    host = load_package().load_host()
    cfg, weights, b = serve_setup(host, Q4, Q8, n_seq, seed=555, max_ctx=96)
    prompts = [list(host.synthetic_tokens(3 + (7 * i) % 40, seed=300 + i, n_vocab=cfg.n_vocab)) for i in range(n_seq)]
    streams = np.arange(n_seq, dtype=np.uint32) * 3 + 5
    got = b.generate_topk(prompts, 80, -1, 40, 0.9, 4242, streams)
    perm = np.random.default_rng(n_seq).permutation(n_seq)
    moved = b.generate_topk([prompts[q] for q in perm], 80, -1, 40, 0.9, 4242, streams[perm])
    for i, q in enumerate(perm):
        assert moved[i].tolist() == got[q].tolist(), (i, q)
    greedy = b.generate(prompts, 80)
    assert sum(g.tolist() != s.tolist() for g, s in zip(greedy, got)) > n_seq // 2
    srv, _ = b.serve_topk(prompts, 80, -1, [0 if q % 2 else 40 for q in range(n_seq)], 0.9, 4242)
    for q in range(1, n_seq, 2):
        assert srv[q].tolist() == greedy[q].tolist(), q
    b.close()


def test_cli_top_k_prints_the_ids_of_the_device_sampler(hip, tmp_path):
    import subprocess
    from test_cli_gpu import write_vocab
    pkg = load_package()
    host = pkg.load_host()
    cfg = host.default_config(4, 3)
    ckpt, vocab = str(tmp_path / "tinyllama.q4.gten"), str(tmp_path / "vocab.bin")
    host.write_gten(cfg, 4242, ckpt)
    write_vocab(vocab)
    n_pred = 48
    r = subprocess.run([pkg.build.HOST_CLI, "-q4", "--ids", "--seed", "7", "--topk", "40", "--temp", "0.9", "--npred", str(n_pred),
                        "--model", ckpt, "--tokenizer", vocab, "-p", "hello world"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(x) for x in r.stdout.split()]
    prompt = host.tokenizer(vocab).encode("hello world")
    cfg.max_ctx = n_pred
    m = host.model(cfg)
    m.load_gten(ckpt)
    want = m.generate_topk(prompt, n_pred, 32002, 40, 0.9, 7)
    greedy = m.generate(prompt, n_pred, 32002)
    m.close()
    assert got == want[len(prompt):].tolist() and len(got) > 0
    assert got != greedy[len(prompt):].tolist()
