"""-m gpu: SEVERAL shared prefixes per batch and decoder (DESIGN.md 3.9 "several prefixes"; include/gten_hip_prefixes.h,
include/gten_host_prefixes.h).  A prompt takes the longest registered prefix it begins with; its slot reads that prefix's full
chunks from the decoder's one copy of THAT prefix.  The contract is the one of a single prefix: ids, logits and cache rows are
the bytes of processing every prompt whole and decoding on private copies.  So every comparison is EQUALITY of ids and logits
bytes, and the reference side is the same build with NO prefix registered and gten_hip_set_prefix_decode_shared(0)."""
import numpy as np
import pytest

from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from helpers import F16, Q4, Q8, tiny_config
from test_model_gpu import host_cfg
from test_prefix_decode_gpu import begin_streams, foreign_bytes, prefill_all, ragged_steps, toks
import prefixes_ref

pytestmark = pytest.mark.gpu

MAX_CTX = 768                 # three chunks of 256 positions
N_PREFIXES = 8
_batches = {}


def new_batch(mode, n_seq=16):
    """2 layers, 4 heads / 2 kv heads, d_head 64 (the model of tests/test_prefix_decode_gpu.py)"""
    wd, ad = {"q4": (Q4, Q8), "f16": (F16, F16)}[mode]
    host = load_package().load_host()
    cfg = host_cfg(tiny_config(wd, ad, n_heads=4, n_kv_heads=2, n_layers=2, max_ctx=MAX_CTX))
    b = host.batch(cfg, n_seq)
    for i in range(len(cfg.weight_shapes())):
        b.set_weight(i, host.synth_weight(cfg, 777, i))
    return host, cfg, b


def batch_of(mode, n_seq=16):
    key = (mode, n_seq)
    if key not in _batches:
        _batches[key] = new_batch(mode, n_seq)
    return _batches[key]


@pytest.fixture(scope="module", autouse=True)
def _close_batches():
    yield
    for host, _, b in _batches.values():
        host.set_prefix_decode_shared(None)
        b.close()
    _batches.clear()


def clear_all(b):
    for w in range(N_PREFIXES):
        b.set_prefix_at(w, None)


def both_ways(host, b, play):
    """play(False): nothing registered, every sequence on its own copy -- the reference; play(True): the prefixes: (want, got)"""
    out = []
    for on in (False, True):
        clear_all(b)
        host.set_prefix_decode_shared(on)
        try:
            out.append(play(on))
        finally:
            host.set_prefix_decode_shared(None)
            clear_all(b)
    return out


def register(b, on, table):
    """table: {index: ids}, registered on the sharing side only"""
    if on:
        for w, ids in table.items():
            b.set_prefix_at(w, ids)


def views(b, n):
    return [b.prefix_decode_info_at(q) for q in range(n)]


# ---------------------------------------------------------------- 1. three prefixes at once


@pytest.mark.parametrize("mode", ["q4", "f16"])
def test_three_prefixes_at_once(hip, mode):
    host, cfg, b = batch_of(mode)
    A, B, C, D = (toks(host, cfg, n, 100 + n) for n in (256, 270, 520, 40))
    table = {0: A, 1: B, 2: C, 5: D}                              # (D: no full chunk -- nothing may change behind it)
    plan = [(0, 16), (0, 33), (0, 50), (1, 17), (1, 20), (1, 230), (2, 16), (2, 31), (2, 48), (5, 30)]   # (1, 230): 500 ids, crosses 512
    prompts = [table[w] + toks(host, cfg, n, 200 + i) for i, (w, n) in enumerate(plan)]
    expect = [(w, len(table[w]) // 256) if len(table[w]) >= 256 else (-1, 0) for w, _ in plan]
    prompts.append(toks(host, cfg, 300, 300))                     # a stranger
    prompts.append(A + toks(host, cfg, 15, 301))                  # 15 ids of its own: processed whole, shares nothing
    expect += [(-1, 0), (-1, 0)]
    assert prefixes_ref.match([table.get(w, []) for w in range(N_PREFIXES)], prompts[-1]) == -1
    steps = 24

    def play(on):
        foreign_bytes(b, host, cfg, len(prompts), 900)
        register(b, on, table)
        lg = prefill_all(b, list(range(len(prompts))), prompts)
        begin_streams(b, host, cfg, prompts, steps)
        ids = ragged_steps(b, prompts, 1, steps)
        last = np.stack([b.logits(q) for q in range(len(prompts))])
        return lg, ids, last, views(b, len(prompts)), [b.prefixes_info(w)[0] for w in range(N_PREFIXES)]

    want, got = both_ways(host, b, play)
    assert want[3] == [(-1, 0)] * len(prompts) and want[4] == [0] * N_PREFIXES
    assert got[3] == expect, got[3]
    assert got[4] == [len(table.get(w, [])) for w in range(N_PREFIXES)]
    assert np.array_equal(got[0], want[0]), "prompt logits"
    assert got[1] == want[1], "ids per step"
    assert np.array_equal(got[2], want[2]), ("last logits", np.nonzero((got[2] != want[2]).any(axis=1))[0].tolist())


# ---------------------------------------------------------------- 2. the longest match


@pytest.mark.parametrize("ia,ib", [(0, 1), (1, 0)])
def test_longest_match(hip, ia, ib):
    host, cfg, b = batch_of("q4")
    A = toks(host, cfg, 256, 1101)
    B = A + toks(host, cfg, 264, 1102)
    prompts = [B + toks(host, cfg, 20, 1110),                     # begins with B: B, two chunks
               A + toks(host, cfg, 40, 1111),                     # begins with A, not with B: A, one chunk
               B + toks(host, cfg, 10, 1112)]                     # begins with B, 10 ids behind it: falls back to A
    assert prompts[1][:len(B)] != B
    expect = [(ib, 2), (ia, 1), (ia, 1)]

    def play(on):
        foreign_bytes(b, host, cfg, len(prompts), 1150)
        register(b, on, {ia: A, ib: B})
        before = [b.prefixes_info(w)[1] for w in (ia, ib)]
        lg = prefill_all(b, list(range(len(prompts))), prompts)
        begin_streams(b, host, cfg, prompts, 6)
        ids = ragged_steps(b, prompts, 1, 6)
        last = np.stack([b.logits(q) for q in range(len(prompts))])
        return lg, ids, last, views(b, len(prompts)), [b.prefixes_info(w)[1] - n for w, n in zip((ia, ib), before)]

    want, got = both_ways(host, b, play)
    assert got[3] == expect and want[3] == [(-1, 0)] * 3
    assert got[4] == [2, 1] and want[4] == [0, 0]                 # prompts that took the short way behind A, behind B
    assert np.array_equal(got[0], want[0])
    assert got[1] == want[1]
    assert np.array_equal(got[2], want[2])


# ---------------------------------------------------------------- 3. prefixes are independent


@pytest.mark.parametrize("how", ["set", "steps"])
def test_replacing_one_prefix_leaves_the_other_alone(hip, how):
    """sequences 0-2 share prefix 0, 3-5 prefix 1.  Prefix 1 is replaced in place by other ids of the same length (set), or its
    set's rows 199 .. 255 are rewritten by the set's own single-sequence decoder (steps): the shared decoder hears of that
    through its watch only"""
    host, cfg, b = batch_of("q4")
    P0, P1, other = toks(host, cfg, 256, 1201), toks(host, cfg, 256, 1202), toks(host, cfg, 256, 1203)
    prompts = [(P0 if i < 3 else P1) + toks(host, cfg, n, 1210 + i) for i, n in enumerate((16, 40, 21, 33, 18, 47))]
    prompts.append(toks(host, cfg, 290, 1230))

    def play(on):
        foreign_bytes(b, host, cfg, len(prompts), 1250)
        base = [b.prefix_decode_info_at(0, w)[3] for w in (0, 1)]   # (import counts run on from the module's earlier tests)
        register(b, on, {0: P0, 1: P1})
        prefill_all(b, list(range(len(prompts))), prompts, want=False)
        begin_streams(b, host, cfg, prompts, 10)
        ids = ragged_steps(b, prompts, 1, 4)
        before = views(b, len(prompts))
        imports0 = tuple(b.prefix_decode_info_at(0, w)[3] - base[w] for w in (0, 1))
        sharers0 = b.prefix_decode_info_at(0, 0)[4], b.prefix_decode_info_at(0, 1)[4]
        seq_imports0 = b.kv_info()[1]
        if on and how == "set":
            b.set_prefix_at(1, other)
        elif on:
            b.prefix_set_steps(1, P1[:150] + other[150:], 200, 57)
        after = views(b, len(prompts))
        ids += ragged_steps(b, prompts, 5, 10)
        last = np.stack([b.logits(q) for q in range(len(prompts))])
        imports1 = tuple(b.prefix_decode_info_at(0, w)[3] - base[w] for w in (0, 1))
        sharers1 = b.prefix_decode_info_at(0, 0)[4], b.prefix_decode_info_at(0, 1)[4]
        return ids, last, before, after, views(b, len(prompts)), imports0, imports1, sharers0, sharers1, b.kv_info()[1] - seq_imports0

    want, got = both_ways(host, b, play)
    assert got[2] == [(0, 1)] * 3 + [(1, 1)] * 3 + [(-1, 0)] and want[2] == [(-1, 0)] * 7
    assert got[3] == got[4] == [(0, 1)] * 3 + [(-1, 0)] * 4       # sharers of 0 keep their chunks, sharers of 1 are off
    assert got[5] == (1, 1) and got[6] == (1, 1)                  # prefix 0's import count did not move (nobody shares the new 1)
    assert got[7] == (3, 3) and got[8] == (3, 0)
    assert got[9] == 3 and want[9] == 0                           # exactly the sharers of 1 went back to their own rows
    assert got[0] == want[0]
    assert np.array_equal(got[1], want[1])


# ---------------------------------------------------------------- 4. the first use of an index above 0 (and of index 0 after one)


@pytest.mark.parametrize("first,second", [(0, 3), (3, 0)])
def test_first_use_mid_run(hip, first, second):
    """a FRESH decoder takes steps sharing prefix `first` only, then index `second` is set mid-run (the step changes its
    attention instantiation, the graphs captured so far go) and two sequences whose rows begin with its ids are promised to it"""
    host, cfg, ref = batch_of("q4")
    F, S = toks(host, cfg, 256, 1301), toks(host, cfg, 270, 1302)
    prompts = [F + toks(host, cfg, n, 1310 + i) for i, n in enumerate((16, 29, 44))]
    prompts += [S + toks(host, cfg, n, 1320 + i) for i, n in enumerate((18, 35))]
    prompts.append(toks(host, cfg, 280, 1330))

    def play(b, on):
        foreign_bytes(b, host, cfg, len(prompts), 1350)
        register(b, on, {first: F})
        prefill_all(b, list(range(len(prompts))), prompts, want=False)
        begin_streams(b, host, cfg, prompts, 10)
        ids = ragged_steps(b, prompts, 1, 5)
        before = views(b, len(prompts))
        if on:
            b.set_prefix_at(second, S)
            for q in (3, 4):                                      # (their rows [0, 270) are the prefix's rows: processed whole, same bytes)
                assert b.prefixes_decode_share_rc(q, second, len(S)) == 0
        mid = views(b, len(prompts))
        ids += ragged_steps(b, prompts, 6, 10)
        last = np.stack([b.logits(q) for q in range(len(prompts))])
        return ids, last, before, mid, views(b, len(prompts))

    clear_all(ref)
    host.set_prefix_decode_shared(False)
    try:
        want = play(ref, False)
    finally:
        host.set_prefix_decode_shared(None)
    _, _, fresh = new_batch("q4")
    try:
        host.set_prefix_decode_shared(True)
        got = play(fresh, True)
    finally:
        host.set_prefix_decode_shared(None)
        fresh.close()
    assert got[2] == [(first, 1)] * 3 + [(-1, 0)] * 3
    assert got[3] == got[4] == [(first, 1)] * 3 + [(second, 1)] * 2 + [(-1, 0)]      # the sharers of `first` stay on it
    assert want[4] == [(-1, 0)] * 6
    assert got[0] == want[0]
    assert np.array_equal(got[1], want[1])


# ---------------------------------------------------------------- 5. the serving queue


def queue_of(host, cfg, table, count=64):
    out = []
    keys = sorted(table)
    for j in range(count):
        if j % 5 == 4:
            out.append(toks(host, cfg, 10 + (13 * j) % 70, 1700 + j))                  # strangers, some under 16 ids
        else:
            out.append(table[keys[j % len(keys)]] + toks(host, cfg, 12 + (7 * j) % 45, 1700 + j))   # (a few with under 16 own ids)
    return out


@pytest.mark.parametrize("spares", [0, -1])
@pytest.mark.parametrize("schedule", [1, 3])
def test_serve_over_three_prefixes(hip, schedule, spares):
    host, cfg, b = batch_of("q4")
    table = {0: toks(host, cfg, 256, 1601), 2: toks(host, cfg, 270, 1602), 6: toks(host, cfg, 520, 1603)}
    queue = queue_of(host, cfg, table)
    reg = [table.get(w, []) for w in range(N_PREFIXES)]
    matched = [prefixes_ref.match(reg, p) for p in queue]
    per = [sum(1 for m in matched if m == w) for w in range(N_PREFIXES)]
    assert all(per[w] >= 10 for w in table) and matched.count(-1) >= 12 and sum(per) + matched.count(-1) == len(queue)
    b.set_serve_schedule(schedule)
    b.set_serve_spares(spares)

    def play(on):
        register(b, on, table)
        n0 = [b.prefixes_info(w)[1] for w in range(N_PREFIXES)]
        ids, st = b.serve(queue, MAX_CTX, -1, 8, max_new=12)
        return ids, st, [b.prefixes_info(w)[1] - n0[w] for w in range(N_PREFIXES)]

    try:
        want, got = both_ways(host, b, play)
    finally:
        b.set_serve_schedule(0)
        b.set_serve_spares(-1)
    for j in range(len(queue)):
        assert got[0][j].tolist() == want[0][j].tolist(), (schedule, spares, j)
    assert got[1]["new_tokens"] == want[1]["new_tokens"] == 12 * len(queue)
    assert got[2] == per and want[2] == [0] * N_PREFIXES          # per prefix, and together the prompts that matched


# ---------------------------------------------------------------- 6. wide decoders


# 128: the nontemporal instantiations; 256: two lanes of 128 -- counts and indices are one array each over all lanes
@pytest.mark.parametrize("n_seq", [128, 256])
def test_wide_decoders(hip, n_seq):
    host, cfg, b = new_batch("q4", n_seq)
    P = 256
    table = {1: toks(host, cfg, P, 1801), 4: toks(host, cfg, P, 1802)}
    front = lambda q: [toks(host, cfg, P, 1900 + q), table[1], table[4]][q % 3]         # (128 is no multiple of 3)
    prompts = [front(q) + toks(host, cfg, 16 + q % 23, 2100 + q) for q in range(n_seq)]
    held = [0, 1, 2, 64, 127] + ([128, 129, 130, 200, 255] if n_seq > 128 else [])

    def play(on):
        foreign_bytes(b, host, cfg, n_seq, 1850)
        register(b, on, table)
        prefill_all(b, list(range(n_seq)), prompts, want=False)
        begin_streams(b, host, cfg, prompts, 8)
        ids = ragged_steps(b, prompts, 1, 8, held)
        last = np.stack([b.logits(q) for q in held])
        return ids, last, views(b, n_seq), [b.prefix_decode_info_at(0, w)[4] for w in (1, 4)]

    try:
        want, got = both_ways(host, b, play)
    finally:
        b.close()
    assert got[2] == [[(-1, 0), (1, 1), (4, 1)][q % 3] for q in range(n_seq)] and want[2] == [(-1, 0)] * n_seq
    assert got[3] == [sum(1 for q in range(n_seq) if q % 3 == r) for r in (1, 2)] and want[3] == [0, 0]
    assert got[0] == want[0]
    assert np.array_equal(got[1], want[1]), np.nonzero((got[1] != want[1]).any(axis=1))[0].tolist()


# ---------------------------------------------------------------- 7. refusals, and where nothing happens


def test_refusals_and_inert_cases(hip):
    host, cfg, b = batch_of("q4")
    P = 256
    pa, pb = toks(host, cfg, P, 2201), toks(host, cfg, 300, 2202)
    prompts = [pa + toks(host, cfg, 40, 2210), pb + toks(host, cfg, 30, 2211), toks(host, cfg, 60, 2212)]
    clear_all(b)
    host.set_prefix_decode_shared(True)
    try:
        assert b.set_prefix_at_rc(-1, pa) == -1 and b.set_prefix_at_rc(8, pa) == -1                  # which outside 0 .. 7
        assert b.set_prefix_at_rc(2, pa[:15]) == -1 and b.set_prefix_at_rc(2, toks(host, cfg, MAX_CTX - 16, 2203)) == -1
        base = {w: b.prefix_decode_info_at(0, w)[3] for w in (2, 7)}  # (import counts run on from the module's earlier tests)
        b.set_prefix_at(2, pa)
        b.set_prefix_at(7, pb)
        prefill_all(b, [0, 1, 2], prompts, want=False)
        begin_streams(b, host, cfg, prompts, 4)
        ragged_steps(b, prompts, 1, 2)
        assert views(b, 3) == [(2, 1), (7, 1), (-1, 0)]
        assert b.prefixes_decode_share_rc(0, -1, P) != 0 and b.prefixes_decode_share_rc(0, 8, P) != 0
        assert b.prefixes_decode_share_rc(0, 2, P + 1) != 0       # more rows than prefix 2 has
        assert views(b, 3) == [(2, 1), (7, 1), (-1, 0)]           # refusals record nothing
        assert b.prefixes_decode_share_rc(0, 3, P) != 0           # index 3 is not set
        assert b.prefixes_decode_share_rc(2, 2, P) != 0           # sequence 2 holds 62 rows: 256 lie beyond them
        assert b.prefixes_decode_share_rc(2, 2, 62) == 0          # (62 rows: taken, and no full chunk)
        assert views(b, 3) == [(2, 1), (7, 1), (-1, 0)]
        assert b.prefixes_decode_share_rc(1, 7, 0) == 0 and views(b, 3)[1] == (-1, 0)                # withdrawn
        assert b.prefixes_decode_share_rc(1, 7, 300) == 0 and views(b, 3)[1] == (7, 1)               # ... and taken again
        b.set_prefix_at(7, None)                                  # clearing an index takes its sharers off -- and only them
        assert views(b, 3) == [(2, 1), (-1, 0), (-1, 0)]
        assert b.prefix_decode_info_at(0, 7)[2:] == (0, base[7] + 1, 0) and b.prefix_decode_info_at(0, 2)[2:] == (P, base[2] + 1, 1)
        assert b.prefixes_decode_share_rc(1, 7, 16) != 0          # no prefix there
        ragged_steps(b, prompts, 3, 4)
    finally:
        clear_all(b)
        host.set_prefix_decode_shared(None)
    small = host.batch(cfg, 8)                                    # 8 sequences: no shadows, no segmented prompts -- all of it is inert
    try:
        for i in range(len(cfg.weight_shapes())):
            small.set_weight(i, host.synth_weight(cfg, 777, i))
        assert small.set_prefix_at_rc(3, pa) == -2
        assert small.prefixes_decode_share_rc(0, 3, 256) == 0
        assert small.prefix_decode_info_at(0, 3) == (-1, 0, 0, 0, 0)
    finally:
        small.close()


# ---------------------------------------------------------------- 8. index 0 is the prefix of set_prefix


def test_legacy_calls_speak_of_index_zero(hip):
    host, cfg, _ = batch_of("q4")
    prefix = toks(host, cfg, 256, 2301)
    prompts = [prefix + toks(host, cfg, n, 2310 + i) for i, n in enumerate((16, 37))] + [toks(host, cfg, 90, 2320)]
    host.set_prefix_decode_shared(True)
    out = []
    try:
        for legacy in (True, False):
            _, _, b = new_batch("q4")
            try:
                if legacy:
                    b.set_prefix(prefix)
                else:
                    b.set_prefix_at(0, prefix)
                prefill_all(b, list(range(len(prompts))), prompts, want=False)
                begin_streams(b, host, cfg, prompts, 6)
                ids = ragged_steps(b, prompts, 1, 6)
                out.append((ids, b.prefix_info(), b.prefixes_info(0), [b.prefix_decode_info(q) for q in range(3)], views(b, 3)))
                b.set_prefix(None) if not legacy else b.set_prefix_at(0, None)     # (... and either call clears what the other set)
                assert b.prefix_info()[0] == 0 and b.prefixes_info(0)[0] == 0
            finally:
                b.close()
    finally:
        host.set_prefix_decode_shared(None)
    assert out[0] == out[1]
    ids, info, info0, dec, at = out[0]
    assert info[:2] == (256, 2) and info0 == (256, 2, 16 + 37)
    assert [d[:2] for d in dec] == [(256, 1), (256, 1), (256, 0)] and at == [(0, 1), (0, 1), (-1, 0)]
