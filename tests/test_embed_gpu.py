"""-m gpu: embeddings (include/gten_hip_embed.h, include/gten_host_embed.h).

1. gten_hip_pool_rows against tests/embed_ref.py: mean and last un-normalised bit-equal, normalised within 1 f32 ulp (the device's f64
   divide and square root are not pinned to the last bit; the rest is exact).  Q8 and f16 rows; n_embd 32 / 288 / 2048; minimal and
   padded pitch; segments of 1 / 63 / 64 / 65 / 128 / 129 / 2048 rows; 1, 3 and 32 segments; zero rows, -0, f16 at +-60000 over 2048
   rows, Q8 blocks with delta 0; bad arguments.
2. hidden_many against the oracle: the library and the oracle hold the same synthetic weights, but an lm_head whose first n_embd rows
   are the identity in the weight dtype, so the oracle's logits(tokens[:t + 1], 0)[:n_embd] are its final-norm row t times a known
   constant.  Compared in the band of tests/test_golden_gpu.py.
3. hidden_many of a text that goes alone, pushed through gten_hip_matmul_2d with the model's lm_head: logits_all, bit for bit.
4. embed_many: embed_ref's pooling of hidden_many; a text's bytes do not depend on its group; `layer`; no stale scratch.
5. refusals, after each of which the model still embeds.
"""
import numpy as np
import pytest

import embed_ref as ref
from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from helpers import F16, F32, MODES, Q4, Q8, tiny_config

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_pooled(got, want, norm, what):
    """un-normalised: the same bits (signs of zero included); normalised: within 1 ulp"""
    assert got.shape == want.shape and np.isfinite(got).all(), what
    if not norm:
        assert np.array_equal(bits(got), bits(want)), (what, int((bits(got) != bits(want)).sum()))
    else:
        u = ref.ulps(got, want)
        assert u.max() <= 1, (what, int(u.max()), int((u > 1).sum()))


def check_pool(hip, rows, dtype, n_embd, starts, pad=0, what=""):
    """rows: uint8 [R][row bytes] -> a device matrix of pitch row bytes + pad; all four (pooling, normalize) pairs against the reference"""
    rb = ref.row_bytes(dtype, n_embd)
    assert rows.shape[1] == rb and starts[-1] <= rows.shape[0]
    pitch = rb + pad
    mat = np.zeros((rows.shape[0], pitch), np.uint8)
    mat[:, :rb] = rows
    mat[:, rb:] = 0xA5                                               # bytes between rows are nobody's values
    dev = hip.upload(mat)
    for pooling in ("mean", "last"):
        for norm in (False, True):
            got = hip.pool_rows(dev, dtype, pitch, n_embd, starts, pooling, norm)
            want = ref.pool_rows(rows, dtype, starts, pooling, norm)
            assert_pooled(got, want, norm, (what, dtype, n_embd, pad, pooling, norm))
    dev.free()


def f16_rows(r, n, n_embd, scale=1.0):
    return (r.standard_normal((n, n_embd)) * scale).astype(np.float16).view(np.uint8).reshape(n, -1)


def q8_rows(r, n, n_embd):
    """random quants; deltas of mixed magnitude, f16 denormals among them"""
    delta = (r.uniform(0.0, 0.05, (n, n_embd // 32)) * r.choice([1.0, 1e-3, 1e-6], (n, n_embd // 32))).astype(np.float16)
    return ref.pack_q8(r.integers(-127, 128, (n, n_embd)), delta)


def starts_of(lengths, first=0):
    return [first] + [first + int(x) for x in np.cumsum(lengths)]


@pytest.mark.parametrize("dtype", [Q8, F16])
def test_pool_rows_against_reference(hip, dtype):
    r = np.random.default_rng(dtype)
    make = q8_rows if dtype == Q8 else f16_rows
    # every segment length at which the chunking takes another path, one of them of 2048 rows; 288 columns are no multiple of 64 or 256;
    # a pitch that leaves every row at another offset from 16 bytes
    lengths = [1, 63, 64, 65, 128, 129, 2048]
    rows = make(r, sum(lengths), 288)
    check_pool(hip, rows, dtype, 288, starts_of(lengths), pad=6, what="lengths")
    check_pool(hip, rows, dtype, 288, starts_of(lengths), pad=0, what="lengths, minimal pitch")
    # 32 segments of one block per row
    lengths = [int(x) for x in r.integers(1, 70, 32)]
    check_pool(hip, make(r, sum(lengths), 32), dtype, 32, starts_of(lengths), pad=0, what="32 segments")
    check_pool(hip, make(r, sum(lengths), 32), dtype, 32, starts_of(lengths), pad=2, what="32 segments, padded")
    # the model's width: three segments, then one that does not begin at row 0
    rows = make(r, 200, 2048)
    check_pool(hip, rows, dtype, 2048, starts_of([65, 1, 130]), pad=0, what="3 segments")
    check_pool(hip, rows, dtype, 2048, starts_of([65, 1, 130]), pad=16, what="3 segments, padded")
    check_pool(hip, rows, dtype, 2048, starts_of([129], first=5), pad=0, what="1 segment")


@pytest.mark.parametrize("dtype", [Q8, F16])
def test_pool_rows_at_the_widest_row(hip, dtype):
    """n_embd 8192, the cap: 32 tiles per chunk, and last pooling's largest LDS request (m and the staged row: 49184 bytes for f16 rows,
    above 48 KB and inside the 64 KB a workgroup may have), at an aligned and at the worst pitch"""
    r = np.random.default_rng(100 + dtype)
    rows = (q8_rows if dtype == Q8 else f16_rows)(r, 73, 8192)
    check_pool(hip, rows, dtype, 8192, [0, 3, 73], pad=0, what="8192 columns")
    check_pool(hip, rows, dtype, 8192, [0, 3, 73], pad=14, what="8192 columns, padded")


def test_pool_rows_special_values(hip):
    r = np.random.default_rng(11)
    E = 288
    # a segment of all-zero rows between ordinary ones: a zero vector, not NaN
    for dtype in (Q8, F16):
        rows = (q8_rows if dtype == Q8 else f16_rows)(r, 150, E)
        rows[70:140] = 0
        check_pool(hip, rows, dtype, E, [0, 70, 140, 150], pad=4, what="zero rows")
        dev = hip.upload(rows)
        for pooling in ("mean", "last"):
            got = hip.pool_rows(dev, dtype, ref.row_bytes(dtype, E), E, [0, 70, 140, 150], pooling, True)
            assert np.array_equal(bits(got[1]), np.zeros(E, np.uint32))                      # +0, every one
    # rows holding -0: f16 0x8000; Q8 q = 0 under a negative delta, a negative q under delta 0 (and delta -0)
    h = f16_rows(r, 130, E)
    hv = h.view(np.uint16)
    hv[:, ::3] = 0x8000
    hv[5:70, 1::3] = 0x8000
    check_pool(hip, h, F16, E, [0, 1, 66, 130], pad=2, what="f16 -0")
    check_pool(hip, np.full((70, E), 0x8000, np.uint16).view(np.uint8), F16, E, [0, 1, 66, 70], what="f16 all -0")
    q = r.integers(-127, 128, (130, E))
    d = r.uniform(-0.05, 0.05, (130, E // 32)).astype(np.float16)
    q[:, ::5] = 0
    d[::2, 0] = 0.0
    d[1::2, 1] = -0.0
    d[40:110, 2] = 0.0
    check_pool(hip, ref.pack_q8(q, d), Q8, E, [0, 1, 66, 130], pad=2, what="q8 -0 and delta 0")
    # Q8 rows whose every delta is 0
    check_pool(hip, ref.pack_q8(r.integers(-127, 128, (66, 64)), np.zeros((66, 2), np.float16)), Q8, 64, [0, 65, 66], what="q8 delta 0")
    # f16 at +-60000 over 2048 rows (a chunk's sum reaches 3.8e6, far inside f32)
    big = (r.choice([-60000.0, 60000.0], (2048, 64)) * r.choice([1.0, 0.999], (2048, 64))).astype(np.float16).view(np.uint8).reshape(2048, -1)
    check_pool(hip, big, F16, 64, [0, 2048], what="f16 +-60000")
    check_pool(hip, np.abs(big.view(np.float16)).view(np.uint8), F16, 64, [0, 2048], what="f16 +60000")


def test_pool_rows_bad_arguments(hip):
    E = 64
    rb = ref.row_bytes(Q8, E)
    dev = hip.upload(np.zeros((4200, rb), np.uint8))
    ok = lambda **kw: hip.pool_rows_rc(dev, kw.get("dtype", Q8), kw.get("pitch", rb), kw.get("n_embd", E), kw.get("starts", [0, 10, 20]),  # noqa: E731
                                       kw.get("pooling", "mean"), True)
    assert ok() == 0
    assert ok(starts=[0]) < 0                                        # T = 0
    assert ok(starts=list(range(34))) < 0                            # T = 33
    assert ok(starts=list(range(33))) == 0                           # T = 32
    assert ok(n_embd=16, pitch=4096) < 0 and ok(n_embd=8224, pitch=16384) < 0 and ok(n_embd=48) < 0
    assert ok(starts=[0, 10, 10]) < 0 and ok(starts=[0, 10, 5]) < 0  # a segment of 0 rows, of fewer
    assert ok(starts=[0, 2049]) < 0 and ok(starts=[0, 2048]) == 0    # 2049 rows
    assert ok(starts=[-1, 5]) < 0
    assert ok(pitch=rb - 2) < 0 and ok(pitch=rb + 1) < 0             # below the row size; rows off the 2-byte grid
    assert ok(dtype=F32) < 0 and ok(dtype=Q4) < 0
    assert ok(pooling=2) < 0 and ok(pooling=-1) < 0
    assert hip.pool_rows_rc(None, Q8, rb, E, [0, 10]) < 0
    assert hip._pool_rows(dev.ptr, Q8, rb, E, None, 1, 0, 1, dev.ptr) < 0
    hip.sync()
    got = hip.pool_rows(dev, Q8, rb, E, [0, 10, 20], "mean", True)   # and the operator still works
    assert np.array_equal(bits(got), np.zeros((2, E), np.uint32))


# ---- the model layer

def host_cfg(c):
    pkg = load_package()
    return pkg.HostConfig(**{k: getattr(c, k) for k, _ in c._fields_})


HEAD_CONST = {"f16": 1.0, "q8": 127 * float(np.float16(1 / 127)), "q4": 7 * float(np.float16(1 / 7))}     # q * f16(delta) of a quantised 1


def identity_head(oracle, cfg, wd):
    """an lm_head whose first n_embd rows are the identity, the rest zero, in the weight dtype's storage form"""
    eye = np.zeros((cfg.n_vocab, cfg.n_embd), np.float32)
    eye[: cfg.n_embd] = np.eye(cfg.n_embd, dtype=np.float32)
    return oracle.quantize_weight(eye, wd)


@pytest.mark.oracle_parity
@pytest.mark.parametrize("name,wd,ad", MODES())
def test_hidden_rows_against_oracle(hip, oracle, name, wd, ad):
    """In q8 / q4 the oracle's lm_head reads the final norm's Q8 row as it stands (it does not requantise it: on the CPU its matmul_2d of Q8
    rows with this head returns dequantised row * constant bit for bit, tests/test_embed_cpu.py), so the comparison is with the oracle's
    own row in every mode."""
    from test_golden_gpu import band
    host = load_package().load_host()
    ocfg = tiny_config(wd, ad, n_heads=4, n_kv_heads=2, max_ctx=512)
    assert ocfg.n_vocab == 512 and ocfg.n_embd == 256
    cfg = host_cfg(ocfg)
    gm, om = host.model(cfg), oracle.model(ocfg)
    last = gm.n_weights() - 1
    for i in range(gm.n_weights()):
        w = host.synth_weight(cfg, 9100, i) if i < last else identity_head(oracle, ocfg, wd)
        gm.set_weight(i, w); om.set_weight(i, w)
    texts = [host.synthetic_tokens(n, seed=n, n_vocab=cfg.n_vocab) for n in (17, 100, 300)]     # 17: the shortest that is grouped
    assert host.embed_plan([len(t) for t in texts]) == ([0, 0, 0], [0])
    hidden = gm.hidden_many(texts)
    c = np.float32(HEAD_CONST[name])
    for toks, (rows, dt) in zip(texts, hidden):
        assert dt == ad and rows.shape == (len(toks), ref.row_bytes(ad, cfg.n_embd))
        x = gm.rows_to_f32(rows, dt)
        assert np.array_equal(bits(x), bits(ref.rows_to_f32(rows, dt)))
        for t in sorted(set(np.linspace(0, len(toks) - 1, 8).astype(int).tolist()) | {0, len(toks) - 1}):
            lg = np.asarray(om.logits(list(toks[: t + 1]), 0), np.float64)
            assert (lg[cfg.n_embd:] == 0).all()
            want = lg[: cfg.n_embd]
            band(name, (x[t] * c).astype(np.float64) - want, float(want.std()))
    gm.close(); om.close()


@pytest.mark.parametrize("name,wd,ad", MODES())
def test_hidden_rows_give_the_library_logits(hip, name, wd, ad):
    """a text of 9 ids goes alone, through final_rows: its rows through the operator with the model's lm_head are logits_all's bits"""
    host = load_package().load_host()
    cfg = host_cfg(tiny_config(wd, ad, n_heads=4, n_kv_heads=2, max_ctx=512))
    gm = host.model(cfg)
    for i in range(gm.n_weights()):
        gm.set_weight(i, host.synth_weight(cfg, 9100, i))
    toks = host.synthetic_tokens(9, seed=4, n_vocab=cfg.n_vocab)
    assert host.embed_plan([9]) == ([0], [1])
    (rows, dt), = gm.hidden_many([toks])
    V, E = cfg.n_vocab, cfg.n_embd
    head = host.synth_weight(cfg, 9100, gm.n_weights() - 1).reshape(V, -1)
    out = hip.upload(np.zeros((9, V), np.float32))
    hip.matmul_2d(hip.upload(rows), dt, hip.upload_weight(head, wd, V, E), wd, out, F32, 9, E, V, 0)
    got = out.download(np.float32, (9, V))
    assert np.array_equal(bits(got), bits(gm.logits_all(toks, 0)))
    gm.close()


def check_embed_many(gm, texts):
    """embed_many is embed_ref's pooling of hidden_many on the same texts"""
    hidden = gm.hidden_many(texts)
    xs = [ref.rows_to_f32(rows, dt) for rows, dt in hidden]
    for pooling in ("mean", "last"):
        for norm in (False, True):
            got = gm.embed_many(texts, pooling, norm)
            want = np.stack([ref.pool(x, pooling, norm) for x in xs])
            assert_pooled(got, want, norm, (pooling, norm))


@pytest.mark.parametrize("name,wd,ad", MODES())
def test_embed_many_tiny_model(hip, name, wd, ad):
    host = load_package().load_host()
    ocfg = tiny_config(wd, ad, n_heads=4, n_kv_heads=2, max_ctx=512, n_layers=3)
    cfg = host_cfg(ocfg)
    gm = host.model(cfg)
    ws = [host.synth_weight(cfg, 77, i) for i in range(gm.n_weights())]
    for i, w in enumerate(ws):
        gm.set_weight(i, w)
    texts = [host.synthetic_tokens(n, seed=10 + n, n_vocab=cfg.n_vocab) for n in (17, 100, 300, 9, 64, 65, 1, 129)]
    check_embed_many(gm, texts)
    assert np.array_equal(bits(gm.embed(texts[1])), bits(gm.embed_many(texts)[1]))
    # layer L: the bytes a model of L layers with the same leading weights and the same final norm gives by default
    full = {L: (gm.hidden_many(texts, layer=L), gm.embed_many(texts, "mean", True, layer=L), gm.embed_many(texts, "last", False, layer=L))
            for L in (0, 1, 2, 3)}
    for L in (1, 2, 3):
        lcfg = host_cfg(tiny_config(wd, ad, n_heads=4, n_kv_heads=2, max_ctx=512, n_layers=L))
        lm = host.model(lcfg)
        for i, w in enumerate(ws[: 1 + 9 * L] + ws[-2:]):
            lm.set_weight(i, w)
        hid, mean, last = full[L]
        for (a, _), (b, _) in zip(hid, lm.hidden_many(texts)):
            assert np.array_equal(a, b), L
        assert np.array_equal(bits(mean), bits(lm.embed_many(texts, "mean", True))), L
        assert np.array_equal(bits(last), bits(lm.embed_many(texts, "last", False))), L
        lm.close()
    for (a, _), (b, _) in zip(full[0][0], full[3][0]):                # 0 and n_layers: the model's own output
        assert np.array_equal(a, b)
    assert np.array_equal(bits(full[0][1]), bits(full[3][1]))
    assert not np.array_equal(bits(full[1][1]), bits(full[3][1])) and not np.array_equal(bits(full[2][1]), bits(full[3][1]))
    gm.close()


@pytest.fixture(scope="module")
def full_q4(hip):
    host = load_package().load_host()
    m = host.model(host.default_config(Q4, Q8))
    m.load_synthetic(2024)
    yield host, m
    m.close()


def test_embed_many_groups(full_q4):
    """the shape of tests/test_score_gpu.py::test_score_many_groups: 40 texts over 4096 rows"""
    host, m = full_q4
    r = np.random.default_rng(7)
    texts = [host.synthetic_tokens(int(n), seed=100 + i, n_vocab=32003) for i, n in enumerate(r.integers(16, 240, 40))]
    texts[5] = host.synthetic_tokens(300, seed=99, n_vocab=32003)
    assert sum(len(t) for t in texts) > 4096 and len(host.embed_plan([len(t) for t in texts])[1]) >= 2
    check_embed_many(m, texts)
    tgt = texts[5]
    for pooling, norm in (("mean", True), ("last", False)):
        alone = m.embed(tgt, pooling, norm)
        three = m.embed_many([texts[0], tgt, texts[1]], pooling, norm)
        every = m.embed_many(texts, pooling, norm)
        assert np.array_equal(bits(three[1]), bits(alone)) and np.array_equal(bits(every[5]), bits(alone))
        # a short text (alone, through the model's own operators) beside grouped ones: what embed gives it
        short = host.synthetic_tokens(9, seed=1, n_vocab=32003)
        mix = m.embed_many([texts[0], short, tgt], pooling, norm)
        assert np.array_equal(bits(mix[1]), bits(m.embed(short, pooling, norm))) and np.array_equal(bits(mix[2]), bits(alone))
        assert np.array_equal(bits(mix[0]), bits(every[0]))
    # generation in between, a larger call before: no stale scratch
    want = m.embed(tgt)
    ids = m.generate(texts[3][:20], 40)
    assert len(ids) == 40
    m.embed_many(texts[:12])
    assert np.array_equal(bits(m.embed(tgt)), bits(want))
    assert np.array_equal(m.generate(texts[3][:20], 40), ids)          # and the model generates as before


def test_embed_refusals(full_q4):
    host, m = full_q4
    toks = host.synthetic_tokens(20, seed=2, n_vocab=32003)
    want = m.embed(toks)

    def refused(texts, what, **kw):
        rc, _ = m.embed_many_rc(texts, **kw)
        assert rc < 0 and what in host.embed_error(), (rc, host.embed_error())
        hid = {k: v for k, v in kw.items() if k == "layer"}
        if hid or not kw:
            assert m.hidden_many_rc(texts, **hid)[0] < 0
        assert np.array_equal(bits(m.embed(toks)), bits(want)) and host.embed_error() == ""     # the model still embeds

    refused([toks, toks[:0]], "empty")
    refused([], "no texts")
    refused([toks, host.synthetic_tokens(2049, seed=3, n_vocab=32003)], "over min(2048")
    bad = toks.copy(); bad[7] = 32003
    refused([toks, bad], "outside [0, n_vocab)")
    bad[7] = -1
    refused([bad], "outside [0, n_vocab)")
    refused([toks], "layer", layer=-1)
    refused([toks], "layer", layer=23)
    refused([toks], "pooling", pooling=2)
    refused([toks], "pooling", pooling=-1)
    # a smaller context bounds the texts
    cfg = host_cfg(tiny_config(Q8, Q8, n_heads=4, n_kv_heads=2, max_ctx=128))
    tm = host.model(cfg)
    tm.load_synthetic(3)
    fits, over = host.synthetic_tokens(128, seed=5, n_vocab=cfg.n_vocab), host.synthetic_tokens(129, seed=5, n_vocab=cfg.n_vocab)
    assert tm.embed_many_rc([fits, over])[0] < 0 and "max_ctx" in host.embed_error()
    assert tm.hidden_many_rc([over])[0] < 0
    assert tm.embed_many_rc([fits], layer=3)[0] < 0                    # two layers
    assert np.isfinite(tm.embed_many([fits, fits[:9]])).all()
    tm.close()


def test_cli_embed_matches_embed_many(hip, tmp_path):
    """--embed FILE: one text per line as BOS + plain BPE ids, one line of %.9g values per text -- embed_many's floats exactly"""
    import subprocess
    from test_cli_gpu import write_vocab
    pkg = load_package()
    host = pkg.load_host()
    cfg = host.default_config(Q4, Q8)
    ckpt, vocab, path = str(tmp_path / "tinyllama.q4.gten"), str(tmp_path / "vocab.bin"), str(tmp_path / "texts.txt")
    host.write_gten(cfg, 5151, ckpt)
    write_vocab(vocab)
    r = np.random.default_rng(4)
    lines = [" ".join("".join(r.choice(list("abcdefghij"), int(r.integers(1, 7)))) for _ in range(n)) for n in (40, 2, 90, 11)]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    tok = host.tokenizer(vocab)
    texts = [[1] + list(tok.encode(ln, chat_template=False)) for ln in lines]
    assert min(len(t) for t in texts) < 16 < max(len(t) for t in texts)                    # one goes alone, others share a group
    cfg.max_ctx = 512
    m = host.model(cfg)
    m.load_gten(ckpt)
    for flags, kw in (([], {}), (["--pooling", "last", "--no-normalize", "--layer", "3"], dict(pooling="last", normalize=False, layer=3))):
        res = subprocess.run([pkg.build.HOST_CLI, "-q4", "--embed", path, "--ctx", "512", "--model", ckpt, "--tokenizer", vocab] + flags,
                             capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-2000:]
        got = np.array([[float(v) for v in ln.split()] for ln in res.stdout.strip().splitlines()], dtype=np.float32)
        want = m.embed_many(texts, **kw)
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), flags
    m.close()
