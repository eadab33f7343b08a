"""-m gpu: prompts that share a prefix (include/gten_hip_prefix.h, include/gten_host_prefix.h).  The prefix is
processed once; a prompt that begins with it is computed from its own first id on.  Every comparison here is byte or id
EQUALITY against the unchanged whole-prompt path on the same build: rows of a segmented call do not depend on each other,
so the short way has nothing to be approximately right about."""
import numpy as np
import pytest

from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from helpers import F16, Q4, Q8, act_rows, rng, row_bytes, tiny_config
from test_block_rows_gpu import alloc_acts, make_block
from test_model_gpu import host_cfg

pytestmark = pytest.mark.gpu

E, H, KVH, F = 256, 4, 2, 512
SUFFIXES = (16, 17, 33, 50)          # 17 and 33: partial row tiles
COMPARED = ("k", "v", "attn_out", "h", "out")


# ---------------------------------------------------------------- 1. operator level

_blocks = {}


def block_of(hip, oracle, wd):
    """one AttentionBlock's weights per weight dtype, shared by the cases"""
    if wd not in _blocks:
        _blocks[wd] = make_block(hip, oracle, rng(900 + wd), wd, E, H, KVH, F, 0)
    return _blocks[wd]


def gather(rows2d, starts, lens):
    return np.concatenate([rows2d[s:s + n] for s, n in zip(starts, lens)])


# P: the boundary between the two K / V sources inside a 16-lane column group (40), at a 256-position tile edge (256), inside a
# 64-position V sub-tile of the second tile (270), and the smallest prefix (16)
@pytest.mark.parametrize("P", [16, 40, 256, 270])
@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("wd", [Q4, Q8, F16])
def test_prefixed_block_rows_leave_the_whole_prompts_bytes(hip, oracle, wd, exact, P):
    ad = F16 if wd == F16 else Q8
    w, widths = block_of(hip, oracle, wd)
    r = rng(1000 + P)
    pre_rows, _ = act_rows(oracle, r, P, E, ad)
    suf_rows = [act_rows(oracle, r, n, E, ad)[0] for n in SUFFIXES]
    whole = np.concatenate([np.concatenate([pre_rows, s]) for s in suf_rows])
    n_whole = whole.shape[0]
    w_starts = [0]
    for n in SUFFIXES:
        w_starts.append(w_starts[-1] + P + n)
    ints = dict(adtype=ad, wdtype=wd, n_embd=E, n_heads=H, n_kv_heads=KVH, n_ffn=F)
    hip.set_prefill_exact(exact)
    try:
        # the prompts processed whole: segments of one row matrix
        a_whole = alloc_acts(hip, widths, n_whole, 0, ad)
        bufs = dict(w)
        bufs.update(a_whole)
        bufs["inp"] = hip.upload(whole)
        hip.set_row_segments(w_starts)
        assert hip.block_rows(n_whole, 0, ints, bufs)
        # the prefix alone, as one segment: its K / V rows
        a_pre = alloc_acts(hip, widths, P, 0, ad)
        bufs = dict(w)
        bufs.update(a_pre)
        bufs["inp"] = hip.upload(pre_rows)
        hip.set_row_segments([0, P])
        assert hip.block_rows(P, 0, ints, bufs)
        # what follows the prefix, the short way
        n_suf = sum(SUFFIXES)
        s_starts = [0]
        for n in SUFFIXES:
            s_starts.append(s_starts[-1] + n)
        a_got = alloc_acts(hip, widths, n_suf, 0x5a, ad)
        bufs = dict(w)
        bufs.update(a_got)
        bufs["inp"] = hip.upload(np.concatenate(suf_rows))
        hip.set_row_segments(s_starts)
        assert hip.block_rows_prefixed(n_suf, ints, bufs, a_pre["k"], a_pre["v"], P)
        hip.sync()
        for name in ("k", "v"):
            rb = row_bytes(ad, widths[name])
            wh = a_whole[name].download(nbytes=n_whole * rb).reshape(n_whole, rb)
            assert np.array_equal(a_pre[name].download(nbytes=P * rb).reshape(P, rb), wh[:P]), ("the prefix's own rows", name)
        for name in COMPARED:
            rb = row_bytes(ad, widths[name])
            wh = a_whole[name].download(nbytes=n_whole * rb).reshape(n_whole, rb)
            want = gather(wh, [s + P for s in w_starts[:-1]], SUFFIXES)
            got = a_got[name].download(nbytes=n_suf * rb).reshape(n_suf, rb)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, (name, P, exact, "rows that differ", bad[:8].tolist(), int(bad.size))
    finally:
        hip.set_row_segments(None)
        hip.set_prefill_exact(False)


def test_prefixed_block_rows_refusals(hip, oracle):
    pkg = load_package()
    w, widths = block_of(hip, oracle, Q8)
    a = alloc_acts(hip, widths, 64, 0, Q8)
    pre = alloc_acts(hip, dict(k=widths["k"], v=widths["v"]), 2048, 0, Q8)
    bufs = dict(w)
    bufs.update(a)
    bufs["inp"] = hip.upload(act_rows(oracle, rng(3), 64, E, Q8)[0])
    ints = dict(adtype=Q8, wdtype=Q8, n_embd=E, n_heads=H, n_kv_heads=KVH, n_ffn=F)
    hip.set_row_segments(None)
    with pytest.raises(pkg.GtenHipError):                      # no segments set
        hip.block_rows_prefixed(64, ints, bufs, pre["k"], pre["v"], 32)
    hip.set_row_segments([0, 24, 64])
    try:
        with pytest.raises(pkg.GtenHipError):                  # 2009 + 40 positions
            hip.block_rows_prefixed(64, ints, bufs, pre["k"], pre["v"], 2009)
        with pytest.raises(pkg.GtenHipError):
            hip.block_rows_prefixed(64, ints, bufs, pre["k"], pre["v"], 0)
        assert not hip.block_rows_prefixed(64, dict(ints, n_heads=8), bufs, pre["k"], pre["v"], 32)    # not handled, as block_rows
        assert hip.block_rows_prefixed(64, ints, bufs, pre["k"], pre["v"], 2008)                       # 2008 + 40 = 2048: taken
        hip.sync()
    finally:
        hip.set_row_segments(None)


# ---------------------------------------------------------------- host level

MAX_CTX, N_SEQ = 384, 16
_batches = {}


def batch_of(mode):
    """one 16-sequence batch per configuration for the whole module"""
    if mode not in _batches:
        wd, ad = {"q4": (Q4, Q8), "q8": (Q8, Q8), "f16": (F16, F16)}[mode]
        pkg = load_package()
        host = pkg.load_host()
        cfg = host_cfg(tiny_config(wd, ad, n_heads=4, n_kv_heads=2, n_layers=2, max_ctx=MAX_CTX))
        b = host.batch(cfg, N_SEQ)
        for i in range(len(cfg.weight_shapes())):
            b.set_weight(i, host.synth_weight(cfg, 777, i))
        _batches[mode] = (host, cfg, b)
    return _batches[mode]


@pytest.fixture(scope="module", autouse=True)
def _close_batches():
    yield
    for _, _, b in _batches.values():
        b.close()
    _batches.clear()
    _blocks.clear()


def toks(host, cfg, n, seed):
    return [int(t) for t in host.synthetic_tokens(n, seed=seed, n_vocab=cfg.n_vocab)]


def prefill_and_decode(b, host, cfg, prompts, steps=24):
    """prompts onto sequences 0 .., then `steps` steps of every sequence on given ids: (prompt logits, ids per step, last logits)"""
    lg = b.prefill_many(list(range(len(prompts))), prompts)
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
    return lg, ids, last


@pytest.mark.parametrize("P", [40, 270])
@pytest.mark.parametrize("mode", ["q4", "f16"])
def test_prefill_many_with_and_without_the_prefix(hip, mode, P):
    host, cfg, b = batch_of(mode)
    prefix = toks(host, cfg, P, 100 + P)
    own = [16, 17, 33, 50, 20, 64, 31]
    prompts = [prefix + toks(host, cfg, n, 200 + i) for i, n in enumerate(own)]
    stranger = toks(host, cfg, P + 30, 300)                       # does not begin with the prefix
    assert stranger[:P] != prefix
    short = prefix + toks(host, cfg, 15, 301)                     # 15 ids of its own: goes whole
    prompts = prompts[:3] + [stranger] + prompts[3:5] + [short] + prompts[5:]
    b.set_prefix(None)
    want = prefill_and_decode(b, host, cfg, prompts)
    try:
        b.set_prefix(prefix)
        n0, shared0, rows0 = b.prefix_info()
        assert n0 == P
        got = prefill_and_decode(b, host, cfg, prompts)
        n1, shared1, rows1 = b.prefix_info()
    finally:
        b.set_prefix(None)
    # the short way WAS taken, by exactly the prompts it is for
    assert shared1 - shared0 == len(own)
    assert rows1 - rows0 == sum(own) + len(stranger) + len(short)
    assert np.array_equal(got[0], want[0]), ("prompt logits", np.nonzero((got[0] != want[0]).any(axis=1))[0].tolist())
    assert got[1] == want[1], "ids of the decode steps that read the slots' caches"
    assert np.array_equal(got[2], want[2]), ("last step's logits", np.nonzero((got[2] != want[2]).any(axis=1))[0].tolist())


def test_a_prompt_alone_and_beside_others(hip):
    host, cfg, b = batch_of("q4")
    prefix = toks(host, cfg, 40, 410)
    prompts = [prefix + toks(host, cfg, n, 420 + i) for i, n in enumerate((37, 16, 80, 23))]
    try:
        b.set_prefix(prefix)
        _, s0, _ = b.prefix_info()
        alone = b.prefill_many([0], prompts[:1])
        beside = b.prefill_many([0, 1, 2, 3], prompts)
        one = b.prefill(5, prompts[0])
        _, s1, _ = b.prefix_info()
    finally:
        b.set_prefix(None)
    assert s1 - s0 == 6
    assert np.array_equal(alone[0], beside[0]) and np.array_equal(one, alone[0])


def queue_of(host, cfg, prefix, count=40):
    out = []
    for j in range(count):
        if j % 4 == 3:
            out.append(toks(host, cfg, 10 + (13 * j) % 70, 700 + j))                    # a quarter: their own beginnings, some short
        else:
            out.append(prefix + toks(host, cfg, 12 + (7 * j) % 45, 700 + j))           # (a few with fewer than 16 ids of their own)
    return out


@pytest.mark.parametrize("spares", [0, -1])
@pytest.mark.parametrize("schedule", [1, 3])
def test_serve_with_and_without_the_prefix(hip, schedule, spares):
    host, cfg, b = batch_of("q4")
    prefix = toks(host, cfg, 40, 510)
    queue = queue_of(host, cfg, prefix)
    eligible = sum(1 for p in queue if p[:40] == prefix and len(p) >= 56)
    assert 20 <= eligible < 30
    b.set_serve_schedule(schedule)
    b.set_serve_spares(spares)
    try:
        b.set_prefix(None)
        want, st_w = b.serve(queue, 200, -1, 8, max_new=20)
        b.set_prefix(prefix)
        _, s0, r0 = b.prefix_info()
        got, st_g = b.serve(queue, 200, -1, 8, max_new=20)
        _, s1, r1 = b.prefix_info()
    finally:
        b.set_prefix(None)
        b.set_serve_schedule(0)
        b.set_serve_spares(-1)
    assert s1 - s0 == eligible
    assert r1 - r0 == sum(len(p) for p in queue if len(p) >= 16) - 40 * eligible
    for j in range(len(queue)):
        assert got[j].tolist() == want[j].tolist(), (schedule, spares, j)
    assert st_g["new_tokens"] == st_w["new_tokens"] and st_g["prompt_tokens"] == st_w["prompt_tokens"]


def test_sampled_serve_and_generate_with_and_without_the_prefix(hip):
    host, cfg, b = batch_of("q4")
    prefix = toks(host, cfg, 40, 610)
    queue = queue_of(host, cfg, prefix)
    fixed = [prefix + toks(host, cfg, 16 + 3 * q, 650 + q) for q in range(N_SEQ)]
    b.set_serve_schedule(3)
    try:
        b.set_prefix(None)
        want, _ = b.serve_topk(queue, 200, -1, 8, 0.9, seed=99, slice_steps=8, max_new=20)
        want_gen = b.generate(fixed, 120)
        want_gen_k = b.generate_topk(fixed, 120, -1, 8, 0.9, 7)
        b.set_prefix(prefix)
        _, s0, _ = b.prefix_info()
        got, _ = b.serve_topk(queue, 200, -1, 8, 0.9, seed=99, slice_steps=8, max_new=20)
        _, s1, _ = b.prefix_info()
        got_gen = b.generate(fixed, 120)
        got_gen_k = b.generate_topk(fixed, 120, -1, 8, 0.9, 7)
        _, s2, _ = b.prefix_info()
    finally:
        b.set_prefix(None)
        b.set_serve_schedule(0)
    assert s1 > s0 and s2 - s1 == 2 * N_SEQ
    for j in range(len(queue)):
        assert got[j].tolist() == want[j].tolist(), j
    for q in range(N_SEQ):
        assert got_gen[q].tolist() == want_gen[q].tolist(), q
        assert got_gen_k[q].tolist() == want_gen_k[q].tolist(), q


def test_replacing_the_prefix(hip):
    host, cfg, b = batch_of("q4")
    pa, pb = toks(host, cfg, 48, 801), toks(host, cfg, 19, 802)
    qa = [pa + toks(host, cfg, n, 810 + i) for i, n in enumerate((16, 40, 21))] + [pb + toks(host, cfg, 30, 815)]
    qb = [pb + toks(host, cfg, n, 820 + i) for i, n in enumerate((33, 18))] + [pa + toks(host, cfg, 25, 825)]
    seqs_a, seqs_b = [0, 1, 2, 3], [4, 5, 6]
    b.set_prefix(None)
    _, s_un, r_un = b.prefix_info()
    want_a = b.prefill_many(seqs_a, qa)
    want_b = b.prefill_many(seqs_b, qb)
    n, s, r = b.prefix_info()
    assert n == 0 and s == s_un and r - r_un == sum(map(len, qa)) + sum(map(len, qb))       # no prefix: every row, nobody shares
    try:
        b.set_prefix(pa)
        _, s0, r0 = b.prefix_info()
        got_a = b.prefill_many(seqs_a, qa)
        _, s1, r1 = b.prefix_info()
        b.set_prefix(pb)
        assert b.prefix_info()[0] == len(pb)
        got_b = b.prefill_many(seqs_b, qb)
        _, s2, r2 = b.prefix_info()
    finally:
        b.set_prefix(None)
    assert (s1 - s0, r1 - r0) == (3, sum(map(len, qa)) - 3 * len(pa))
    assert (s2 - s1, r2 - r1) == (2, sum(map(len, qb)) - 2 * len(pb))
    assert np.array_equal(got_a, want_a) and np.array_equal(got_b, want_b)
    n, s3, r3 = b.prefix_info()
    again = b.prefill_many(seqs_a, qa)
    assert n == 0 and b.prefix_info()[1:] == (s3, r3 + sum(map(len, qa))) and np.array_equal(again, want_a)


def test_set_prefix_refusals(hip):
    host, cfg, b = batch_of("q4")
    assert b.set_prefix_rc(toks(host, cfg, 15, 1)) < 0                        # fewer than 16 ids
    assert b.set_prefix_rc(toks(host, cfg, MAX_CTX - 16, 1)) < 0              # n + 17 > max_ctx
    assert b.prefix_info()[0] == 0
    assert b.set_prefix_rc(toks(host, cfg, MAX_CTX - 17, 1)) == 0
    assert b.prefix_info()[0] == MAX_CTX - 17
    assert b.set_prefix_rc(None) == 0 and b.prefix_info()[0] == 0
    small = host.batch(cfg, 8)
    try:
        assert small.set_prefix_rc(toks(host, cfg, 32, 1)) == -2              # 8 sequences: prompts are not processed as segments
        assert small.prefix_info() == (0, 0, 0)
    finally:
        small.close()
