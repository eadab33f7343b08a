"""-m gpu: context shift above the operator (include/gten_host_shift.h) on tiny models.

The cache primitive against tests/shift_ref.py through kv_read; a wide decoder's shadows and a shared prefix copy after a shift
against a decoder created AFTER the shift over the same cache sets (equality: same bytes, same kernels); generation past the window
against a Python loop over the primitives (prefill, steps, batch_shift when shift_plan says so), id for id -- greedy, sampled and
penalised, the loop setting the draw stream and the penalty window's start by the rules the header states; the refusals with their
texts; a session that no longer fits, shifted and served as a continued segment."""
import numpy as np
import pytest

import shift_ref as ref
from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from helpers import F16, Q4, Q8, tiny_config
from test_model_gpu import host_cfg

pytestmark = pytest.mark.gpu

MODES = {"q4": (Q4, Q8), "q8": (Q8, Q8), "f16": (F16, F16)}
GEOMS = {"dh64": dict(n_heads=4, n_kv_heads=2), "dh32": {}}            # 64-wide heads (kv_dim 128), the default 32-wide ones (kv_dim 64)
_made = {}


def made(kind, mode, geom, max_ctx, n_seq=0, **kw):
    """one model (n_seq 0) or batch per configuration for the whole module: (host, cfg, object)"""
    key = (kind, mode, geom, max_ctx, n_seq, tuple(sorted(kw.items())))
    if key not in _made:
        wd, ad = MODES[mode]
        host = load_package().load_host()
        cfg = host_cfg(tiny_config(wd, ad, n_layers=2, max_ctx=max_ctx, **GEOMS[geom], **kw))
        obj = host.batch(cfg, n_seq) if n_seq else host.model(cfg)
        for i in range(len(cfg.weight_shapes())):
            obj.set_weight(i, host.synth_weight(cfg, 777, i))
        _made[key] = (host, cfg, obj)
    return _made[key]


@pytest.fixture(scope="module", autouse=True)
def _close_all():
    yield
    for _, _, obj in _made.values():
        obj.close()
    _made.clear()


def toks(host, cfg, n, seed):
    return [int(t) for t in host.synthetic_tokens(n, seed=seed, n_vocab=cfg.n_vocab)]


def geometry(cfg):
    d_head = cfg.n_embd // cfg.n_heads
    return d_head, d_head * cfg.n_kv_heads


# ---------------------------------------------------------------------------------------------------- the cache primitive

@pytest.mark.parametrize("geom", ["dh64", "dh32"])
@pytest.mark.parametrize("mode", ["q4", "q8", "f16"])
def test_batch_shift_equals_reference_through_kv_read(hip, oracle, mode, geom):
    host, cfg, b = made("batch", mode, geom, 128, 4)       # (never decoded on: the shared decoder takes 64-wide heads only)
    d_head, kv_dim = geometry(cfg)
    rows = [40, 33, 37, 128]
    for q, n in enumerate(rows):
        b.prefill(q, toks(host, cfg, n, 10 + q), want=False)
    before = [[b.kv_read(q, l, 0, 128) for l in range(2)] for q in range(4)]
    assert b.kv_row_bytes() == before[0][0][0].shape[1] == (kv_dim * 2 if cfg.adtype == F16 else kv_dim // 32 * 34)
    info0 = b.shift_info()
    keep, drop = 4, 10
    b.shift([1, 3], [rows[1], rows[3]], keep, drop)
    for q in range(4):
        for l in range(2):
            k, v = b.kv_read(q, l, 0, 128)
            if q in (1, 3):
                wk, wv = ref.shift_ref(oracle, before[q][l][0], before[q][l][1], cfg.adtype, kv_dim, d_head, rows[q], keep, drop)
                assert not np.array_equal(wk, before[q][l][0])
            else:
                wk, wv = before[q][l]                      # sequences not named: not one byte
            assert np.array_equal(k, wk) and np.array_equal(v, wv), (q, l)
    moved = sum(rows[q] - keep - drop for q in (1, 3))
    assert tuple(a - b_ for a, b_ in zip(b.shift_info(), info0)) == (2, moved, 2 * drop)
    # drop 0: half of what lies behind keep
    b.shift([0], [rows[0]], 6)
    k, v = b.kv_read(0, 1, 0, 128)
    wk, wv = ref.shift_ref(oracle, before[0][1][0], before[0][1][1], cfg.adtype, kv_dim, d_head, rows[0], 6, (rows[0] - 6) // 2)
    assert np.array_equal(k, wk) and np.array_equal(v, wv)
    # refusals: nothing fits, a sequence twice, a sequence outside
    assert b.shift_rc([2], [rows[2]], 30, 8) == -1 and "do not fit" in host.shift_error()
    assert b.shift_rc([2, 2], [rows[2]] * 2, 1, 1) == -1 and "twice" in host.shift_error()
    assert b.shift_rc([4], [20], 1, 1) == -1
    k2, _ = b.kv_read(2, 0, 0, 128)
    assert np.array_equal(k2, before[2][0][0])


# ---------------------------------------------------------------------------------------------------- shadows and shared copies

def made_wide(mode, max_ctx, twin):
    """16-sequence batches of one configuration (64-wide heads): what is played on twin 0 is compared with twin 1"""
    key = ("wide", mode, max_ctx, twin)
    if key not in _made:
        wd, ad = MODES[mode]
        host = load_package().load_host()
        cfg = host_cfg(tiny_config(wd, ad, n_layers=2, max_ctx=max_ctx, n_heads=4, n_kv_heads=2))
        b = host.batch(cfg, 16)
        for i in range(len(cfg.weight_shapes())):
            b.set_weight(i, host.synth_weight(cfg, 777, i))
        _made[key] = (host, cfg, b)
    return _made[key]


@pytest.mark.parametrize("mode", ["q4", "f16"])
def test_shifted_sequences_shadows_are_imported_again(hip, mode):
    """Twin 0: a 16-sequence decoder that has stepped on every sequence (its shadows hold the prompts' rows), then a shift of
    sequences 3 and 9, then steps.  Twin 1: the same prompts and the same shift, and only then the first decoder call -- a decoder
    created AFTER the shift over cache sets with the same valid rows.  Logits and ids are equal."""
    P, keep, drop = 40, 4, 12
    runs = []
    for twin in range(2):
        host, cfg, b = made_wide(mode, 128, twin)                  # (twin 1: a batch nobody has decoded on)
        streams = [toks(host, cfg, P + 24, 40 + q) for q in range(16)]
        for q in range(16):
            b.prefill(q, streams[q][:P], want=False)
        if twin == 0:
            for q in range(16):
                b.decode_begin(q, streams[q])
            for n in range(P + 1, P + 5):
                b.decode_step(n, True)
            assert b.kv_info()[0] and b.kv_info()[1] >= 16
        imports0 = b.kv_info()[1] if twin == 0 else 0
        b.shift([3, 9], [P, P], keep, drop)                        # the prompts' rows [0, P) are the valid ones
        ns = [P + 1] * 16
        for q in (3, 9):
            streams[q] = ref.shift_ids(streams[q], keep, drop)
            ns[q] -= drop
        for q in range(16):
            b.decode_begin(q, streams[q])
        out = []
        for t in range(4):
            b.decode_step_ragged([n + t for n in ns], use_graph=(t % 2 == 0))
            out.append([(b.decode_result(q, ns[q] + t), b.logits(q).copy()) for q in (2, 3, 9, 15)])
        if twin == 0:
            assert b.kv_info()[1] - imports0 >= 2                  # the two shifted sequences at the least
        runs.append(out)
    for a, c in zip(*runs):
        for (ia, la), (ic, lc) in zip(a, c):
            assert ia == ic and np.array_equal(la, lc)


@pytest.mark.parametrize("mode", ["q4", "f16"])
def test_a_sharer_of_a_prefix_copy_goes_off_it_when_shifted(hip, mode):
    """Twin 0: four sequences read one copy of a 256-id prefix's chunk; one of them is shifted: it reads its own rows from then on,
    the others stay on the copy.  Twin 1: the same prompts processed whole (no prefix registered, nobody shares), the same shift,
    and only then the first decoder call.  Everyone's logits and ids are equal."""
    P, keep, drop = 256, 4, 20
    runs = []
    for twin in range(2):
        load_package().load_host().set_prefix_decode_shared(True if twin == 0 else None)
        try:
            host, cfg, b = made_wide(mode, 384, twin)
            prefix = toks(host, cfg, P, 77)
            prompts = [prefix + toks(host, cfg, 16 + q, 200 + q) for q in range(4)]
            streams = [p + toks(host, cfg, 12, 5000 + q) for q, p in enumerate(prompts)] + [toks(host, cfg, 16, 6000 + q) for q in range(4, 16)]
            if twin == 0:
                b.set_prefix(prefix)
            b.prefill_many(list(range(4)), prompts, want=False)
            if twin == 0:
                for q in range(16):
                    b.decode_begin(q, streams[q])
                for t in (1, 2):
                    b.decode_step_ragged([len(p) + t for p in prompts] + [t] * 12, use_graph=False)
                assert [b.prefix_decode_info(q)[1] for q in range(4)] == [1, 1, 1, 1]
            b.shift([2], [len(prompts[2])], keep, drop)
            if twin == 0:
                assert [b.prefix_decode_info(q)[1] for q in range(4)] == [1, 1, 0, 1]
            streams[2] = ref.shift_ids(streams[2], keep, drop)
            for q in range(16):
                b.decode_begin(q, streams[q])
            out = []
            for t in (1, 2, 3):
                ns = [len(p) + t for p in prompts] + [t] * 12
                ns[2] -= drop
                b.decode_step_ragged(ns, use_graph=False)
                out.append([(b.decode_result(q, ns[q]), b.logits(q).copy()) for q in range(5)])
            if twin == 0:
                assert [b.prefix_decode_info(q)[1] for q in range(4)] == [1, 1, 0, 1]
                b.set_prefix(None)
            runs.append(out)
        finally:
            load_package().load_host().set_prefix_decode_shared(None)
    for a, c in zip(*runs):
        for (ia, la), (ic, lc) in zip(a, c):
            assert ia == ic and np.array_equal(la, lc)


# ---------------------------------------------------------------------------------------------------- generation past the window

class OnBatch:
    """sequence 0 of a batch as the loop's primitives (the other sequences idle at position 1)"""
    def __init__(self, b, prompt):
        self.b = b
        for q in range(1, b.n_seq):
            b.decode_begin(q, prompt[:2])

    def prefill(self, prompt):
        return self.b.prefill(0, prompt)

    def set_sampling(self, *a):
        self.b.set_sampling(0, *a)

    def set_penalty(self, *a):
        self.b.set_penalty(0, *a)

    def set_cut(self, *a):
        self.b.set_cut(0, *a)

    def shift(self, rows, keep, drop):
        self.b.shift([0], [rows], keep, drop)

    def step(self, view):
        self.b.decode_begin(0, view)
        self.b.decode_step_ragged([len(view)] + [1] * (self.b.n_seq - 1), use_graph=False)
        return self.b.decode_result(0, len(view))


class OnModel:
    """a lone model as the loop's primitives"""
    def __init__(self, m):
        self.m = m

    def prefill(self, prompt):
        return self.m.logits(prompt, 0)

    def set_sampling(self, *a):
        self.m.set_sampling(*a)

    def set_penalty(self, *a):
        self.m.set_penalty(*a)

    def set_cut(self, *a):
        self.m.set_cut(*a)

    def shift(self, rows, keep, drop):
        self.m.shift(rows, keep, drop)

    def step(self, view):
        self.m.decode_begin(view)
        self.m.decode_step(len(view), use_graph=False)
        return self.m.decode_result(len(view))


def loop_over_primitives(hip, host, cfg, on, prompt, total, keep, drop, req):
    """generation past the window by hand: prefill, the first id drawn by the row operator, then step by step; the shift primitive
    when shift_plan says so, the stream and the penalty window's start set by the header's rules.  Returns (ids, (shifts, rows
    moved, rows dropped))"""
    pkg = load_package()
    top_k, temp, seed, stream = req.get("top_k", 0), req.get("temp", 1.0), req.get("seed", 0), req.get("stream", 0)
    rep, freq, pres, last_n = req.get("rep", 1.0), req.get("freq", 0.0), req.get("pres", 0.0), req.get("last_n", 0)
    top_p, min_p = req.get("top_p", 1.0), req.get("min_p", 0.0)
    penalised, cutting = (rep, freq, pres) != (1.0, 0.0, 0.0), (top_p, min_p) != (1.0, 0.0)
    assert not (penalised and cutting)
    P = len(prompt)
    lg = pkg.hipabi.DeviceBuffer.from_numpy(hip, on.prefill(prompt))
    start = 0
    lo = max(start, P - last_n if last_n > 0 else 0)
    if penalised:
        first = int(hip.sample_rows_pen(lg, 1, cfg.n_vocab, cfg.n_vocab, top_k, temp, seed, stream, P, [prompt[lo:P]], rep, freq, pres)[0][0])
    elif cutting:
        first = int(hip.sample_rows_cut(lg, 1, cfg.n_vocab, cfg.n_vocab, top_k, temp, seed, stream, P, top_p, min_p, info=False)[0][0])
    else:
        first = int(hip.sample_rows(lg, 1, cfg.n_vocab, cfg.n_vocab, top_k, temp, seed, stream, P)[0])
    lg.free()
    view, out = list(prompt) + [first], list(prompt) + [first]
    on.set_sampling(top_k, temp, seed, stream)
    if penalised:
        on.set_penalty(rep, freq, pres, start, last_n)
    if cutting:
        on.set_cut(top_p, min_p)                                 # (not bound by position: it holds through every shift)
    counts = [0, 0, 0]
    try:
        while len(out) < total:
            due, k, d, n_ids, rows = host.shift_plan(len(view), len(view) - 1, cfg.max_ctx, keep, drop)
            if due:
                on.shift(len(view) - 1, k, d)
                counts = [counts[0] + 1, counts[1] + len(view) - 1 - k - d, counts[2] + d]
                view = ref.shift_ids(view, k, d)
                assert (len(view), len(view) - 1) == (n_ids, rows)
                start = ref.phi(start, k, d)
                on.set_sampling(top_k, temp, seed, stream + (counts[0] << 24))
                if penalised:
                    on.set_penalty(rep, freq, pres, start, last_n)
            nxt = on.step(view)
            view.append(nxt)
            out.append(nxt)
    finally:
        on.set_sampling(0, 1.0, 0, 0)
        if penalised:
            on.set_penalty(1.0, 0.0, 0.0, 0, 0)
        if cutting:
            on.set_cut(1.0, 0.0)
    return out, tuple(counts)


REQUESTS = {"greedy": {}, "topk": dict(top_k=8, temp=0.8, seed=11, stream=3), "nucleus": dict(top_k=8, temp=0.8, seed=12, top_p=0.8, min_p=0.02), "penalised": dict(top_k=8, temp=0.8, seed=11, rep=1.1, freq=0.1, pres=0.1, last_n=16),
            "penalised_greedy": dict(rep=1.1, freq=0.1, pres=0.1, last_n=16)}


@pytest.mark.parametrize("pair", [(4, 0), (0, 8)], ids=["keep4_half", "keep0_drop8"])
@pytest.mark.parametrize("what", list(REQUESTS))
@pytest.mark.parametrize("mode,geom,on", [("q4", "dh32", "model"), ("q8", "dh64", "batch"), ("f16", "dh64", "batch")])
def test_generate_shifting_equals_a_loop_over_the_primitives(hip, mode, geom, on, what, pair):
    """max_ctx 64, a prompt of 20 ids, 150 new ids: the single model, id for id, and the counts the plan predicts.  The loop runs on
    sequence 0 of a 2-sequence batch (whose ids are a lone model's, bit for bit) where the heads are 64 wide -- the shared decoder
    takes no others -- and on a lone model's own primitives where they are 32 wide."""
    keep, drop = pair
    req = REQUESTS[what]
    host, cfg, m = made("model", mode, geom, 64)
    prompt = toks(host, cfg, 20, 31)
    prims = OnBatch(made("batch", mode, geom, 64, 2)[2], prompt) if on == "batch" else OnModel(m)
    want, counts = loop_over_primitives(hip, host, cfg, prims, prompt, 170, keep, drop, req)
    info0 = m.shift_info()
    got = m.generate_shifting(prompt, 170, keep, drop, **req)
    assert len(got) == 170 and list(got) == want
    assert tuple(a - c for a, c in zip(m.shift_info(), info0)) == counts and counts[0] >= 3
    assert len(set(want[20:])) > 4                               # (not a loop of one id: the comparison says something)


@pytest.mark.parametrize("what", ["greedy", "penalised"])
@pytest.mark.parametrize("mode,geom", [("q4", "dh64"), ("f16", "dh64")])
def test_batch_generate_shifting_equals_the_single_form_per_sequence(hip, mode, geom, what):
    """four ragged prompts in a 4-sequence batch (where a sequence's ids are a lone model's, bit for bit): every sequence shifts at a
    step of its own"""
    req = dict(REQUESTS[what])
    host, cfg, m = made("model", mode, geom, 64)
    _, _, b = made("batch", mode, geom, 64, 4)
    prompts = [toks(host, cfg, n, 50 + n) for n in (20, 9, 33, 63)]
    info0 = b.shift_info()
    got = b.generate_shifting(prompts, 150, 4, 0, streams=[5, 6, 7, 8], **req)
    shifts = 0
    for q, p in enumerate(prompts):
        i0 = m.shift_info()[0]
        want = m.generate_shifting(p, 150, 4, 0, stream=5 + q, **req)
        shifts += m.shift_info()[0] - i0
        assert len(got[q]) == 150 and np.array_equal(got[q], want), q
    assert b.shift_info()[0] - info0[0] == shifts and shifts >= 8


def test_keep_below_zero_is_todays_generation(hip):
    host, cfg, m = made("model", "q4", "dh64", 64)
    _, _, b = made("batch", "q4", "dh64", 64, 4)
    prompts = [toks(host, cfg, n, 50 + n) for n in (20, 9, 33, 40)]
    req = dict(top_k=8, temp=0.8, seed=3, rep=1.2, freq=0.05, pres=0.0, last_n=8, top_p=0.9)
    info0 = (m.shift_info(), b.shift_info())
    for p in prompts[:2]:
        assert np.array_equal(m.generate_shifting(p, 64, -1, **req), m.generate_penalized(p, 64, **req))
        assert np.array_equal(m.generate_shifting(p, 50, -1), m.generate(p, 50))
    want = b.generate_penalized(prompts, 60, **req)
    got = b.generate_shifting(prompts, 60, -1, **req)
    assert all(np.array_equal(a, c) for a, c in zip(got, want))
    assert (m.shift_info(), b.shift_info()) == info0             # nothing shifted


def test_what_is_not_carried_through_a_shift_is_refused(hip):
    host, cfg, m = made("model", "q4", "dh64", 64)
    _, _, b = made("batch", "q4", "dh64", 64, 4)
    p = toks(host, cfg, 20, 1)
    cases = [(dict(n_top=2), "log-prob records"), (dict(table=0), "bias table"), (dict(top_k=4, stream=1 << 24), "stream >= 2^24"),
             (dict(), "fit a full window", 60, 8), (dict(), "fit a full window", 64, 0)]
    for c in cases:
        req, text = c[0], c[1]
        keep, drop = (c[2], c[3]) if len(c) > 2 else (4, 0)
        total, _ = m.generate_shifting_rc(p, 100, keep, drop, **req)
        assert total == -1 and text in host.shift_error(), (c, host.shift_error())
        with pytest.raises(load_package().GtenHipError, match=text.replace("^", r"\^")):
            m.generate_shifting(p, 100, keep, drop, **req)
        breq = {("streams" if k == "stream" else k): ([v] * 4 if k == "stream" else v) for k, v in req.items()}
        rc, _ = b.generate_shifting_rc([p] * 4, 100, keep, drop, **breq)
        assert rc == -1 and text in host.shift_error(), (c, host.shift_error())
    total, _ = m.generate_shifting_rc(toks(host, cfg, 64, 2), 100, 4, 0)
    assert total == -1 and "fills the window" in host.shift_error()
    # a stream just below the bound goes through
    assert len(m.generate_shifting(p, 70, 4, 0, top_k=4, stream=(1 << 24) - 1)) == 70


# ---------------------------------------------------------------------------------------------------- sessions

def test_a_full_session_is_shifted_and_served_as_a_continued_segment(hip):
    host, cfg, b = made_wide("q4", 128, 0)
    b.sessions_reserve(2)
    s = b.session_open()
    try:
        first, _, _ = b.serve_sessions([(s, toks(host, cfg, 100, 9))], 128, -1, 1, 1.0, 5, max_new=26)
        hist = [int(t) for t in first[0]]
        assert len(hist) == 126 and b.session_info(s)[:2] == (126, 125)          # max_ctx - 2 ids
        turn = toks(host, cfg, 8, 19)
        assert b.serve_sessions_rc([(s, turn)], 128, -1, 1, 1.0, 5, max_new=4, stride=160)[0] == -1      # as today: it does not fit
        assert np.array_equal(b.session_ids(s), hist)
        assert b.session_shift_rc(s, 120, 8) == -1 and "do not fit" in host.shift_error()
        k0 = b.shift_info()
        d = host.shift_drop(125, 4, 0)
        b.session_shift(s, 4)
        assert d == 60 and tuple(a - c for a, c in zip(b.shift_info(), k0)) == (1, 125 - 4 - d, d)
        kept = ref.shift_ids(hist, 4, d)
        assert b.session_info(s)[:2] == (126 - d, 125 - d) and np.array_equal(b.session_ids(s), kept)
        before = b.sessions_info()
        ids, _, _ = b.serve_sessions([(s, turn)], 128, -1, 1, 1.0, 5, max_new=4)
        after = b.sessions_info()
        assert [int(t) for t in ids[0][: len(kept) + 8]] == kept + turn and len(ids[0]) == len(kept) + 8 + 4
        assert np.array_equal(b.session_ids(s), ids[0])
        assert after[2] - before[2] == 1 and after[3] - before[3] == 1 and after[5] - before[5] == 125 - d   # a continued segment behind the kept rows
    finally:
        b.session_close(s)


# ---------------------------------------------------------------------------------------------------- the command line

def test_cli_ctx_shift_prints_the_ids_of_generate_shifting(hip, tmp_path):
    """--ctx-shift 4 with -greedy: a window of 40 positions, 110 ids in all, on a synthetic full-size q4 checkpoint (the program
    builds no other model)"""
    import subprocess
    from test_cli_gpu import write_vocab
    pkg = load_package()
    host = pkg.load_host()
    cfg = host.default_config(4, 3)
    ckpt, vocab = str(tmp_path / "tinyllama.q4.gten"), str(tmp_path / "vocab.bin")
    host.write_gten(cfg, 4242, ckpt)
    write_vocab(vocab)
    args = [pkg.build.HOST_CLI, "-q4", "-greedy", "--ids", "--ctx", "40", "--npred", "110", "--model", ckpt, "--tokenizer", vocab, "-p", "hello world"]
    r = subprocess.run(args + ["--ctx-shift", "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(x) for x in r.stdout.split()]
    prompt = host.tokenizer(vocab).encode("hello world")
    cfg.max_ctx = 40
    m = host.model(cfg)
    m.load_gten(ckpt)
    want = m.generate_shifting(prompt, 110, 4, eos=32002)
    shifts = m.shift_info()[0]
    m.close()
    assert got == want[len(prompt):].tolist() and len(want) > 41 and shifts >= 1
    # what does not survive a shift is refused by name, before the checkpoint is read
    r = subprocess.run(args + ["--ctx-shift", "4", "--logprobs", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--logprobs" in r.stderr
    r = subprocess.run(args + ["--ctx-shift", "39,2"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "do not fit" in r.stderr
