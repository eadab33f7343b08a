"""-m gpu: decode slots that share a prefix read ONE copy of its K / V (include/gten_hip_prefix_decode.h,
include/gten_host_prefix_decode.h).  A sequence whose caches begin with the prefix set's rows takes its leading full chunks of
256 positions from the decoder's prefix shadow instead of its own; per (sequence, head, chunk) the arithmetic is the same
operations on the same bytes.  So every comparison here is EQUALITY of ids and logits bytes, and the reference side is the same
build, the same calls, with gten_hip_set_prefix_decode_shared(0): every sequence on its own copy."""
import numpy as np
import pytest

from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from helpers import F16, Q4, Q8, tiny_config
from test_model_gpu import host_cfg

pytestmark = pytest.mark.gpu

MAX_CTX = 768                 # three chunks of 256 positions
_batches = {}


def batch_of(mode, n_seq=16):
    """one batch per (configuration, width) for the whole module: 2 layers, 4 heads / 2 kv heads, d_head 64"""
    key = (mode, n_seq)
    if key not in _batches:
        wd, ad = {"q4": (Q4, Q8), "f16": (F16, F16)}[mode]
        host = load_package().load_host()
        cfg = host_cfg(tiny_config(wd, ad, n_heads=4, n_kv_heads=2, n_layers=2, max_ctx=MAX_CTX))
        b = host.batch(cfg, n_seq)
        for i in range(len(cfg.weight_shapes())):
            b.set_weight(i, host.synth_weight(cfg, 777, i))
        _batches[key] = (host, cfg, b)
    return _batches[key]


@pytest.fixture(scope="module", autouse=True)
def _close_batches():
    yield
    for host, _, b in _batches.values():
        host.set_prefix_decode_shared(None)
        b.close()
    _batches.clear()


def toks(host, cfg, n, seed):
    return [int(t) for t in host.synthetic_tokens(n, seed=seed, n_vocab=cfg.n_vocab)]


def prefill_all(b, slots, prompts, want=True):
    """prefill_many in calls of at most 32 prompts and 4096 ids (what one call takes); the prompts' logits"""
    out, i = [], 0
    while i < len(prompts):
        j, ids = i, 0
        while j < len(prompts) and j - i < 32 and ids + len(prompts[j]) <= 4096:
            ids += len(prompts[j])
            j += 1
        assert j > i
        out.append(b.prefill_many(slots[i:j], prompts[i:j], want=want))
        i = j
    return np.concatenate(out) if want else None


def foreign_bytes(b, host, cfg, n_prompts, seed):
    """other prompts, no shared beginning, onto the same slots and two steps of them: the slots' own shadows then hold
    another context's bytes -- neither zeros nor an earlier copy of the prefix"""
    prompts = [toks(host, cfg, 300 + 7 * (q % 32), seed + q) for q in range(n_prompts)]
    prefill_all(b, list(range(n_prompts)), prompts, want=False)
    for q, p in enumerate(prompts):
        b.decode_begin(q, p + toks(host, cfg, 2, seed + 100 + q))
    for t in (1, 2):
        b.decode_step_ragged([len(p) + t for p in prompts] + [1] * (b.n_seq - n_prompts), use_graph=False)


def begin_streams(b, host, cfg, prompts, steps):
    streams = [list(p) + toks(host, cfg, steps, 5000 + q) for q, p in enumerate(prompts)]
    for q, s in enumerate(streams):
        b.decode_begin(q, s)
    for q in range(len(prompts), b.n_seq):                        # the other sequences step along from position 0
        b.decode_begin(q, toks(host, cfg, steps + 1, 6000 + q))
    return streams


def ragged_steps(b, prompts, first, last, held=None):
    """steps first .. last of every prompt's sequence (graph replay on alternate steps): the ids per step.  Every sequence
    moves on by one position per step, so steps after the first CONTINUE the run: nobody is restarted, nothing is imported
    unless its rows or its promise changed"""
    held = range(len(prompts)) if held is None else held
    ids = []
    for t in range(first, last + 1):
        ns = [len(p) + t for p in prompts] + [t] * (b.n_seq - len(prompts))
        b.decode_step_ragged(ns, use_graph=(t % 2 == 0))
        ids.append([b.decode_result(q, ns[q]) for q in held])
    return ids


def both_ways(host, play):
    """play() with every sequence on its own copy, then with the sharing on: (want, got)"""
    out = []
    for on in (False, True):
        host.set_prefix_decode_shared(on)
        try:
            out.append(play(on))
        finally:
            host.set_prefix_decode_shared(None)               # (the default again)
    return out


# ---------------------------------------------------------------- 1. prefill_many, then ragged decode steps


# P = 40: no full chunk, nothing may change; 256: a workgroup's pair of waves is (shared, own); 270: the boundary lies inside the
# own chunk; 520: two shared chunks, the own one is the third
@pytest.mark.parametrize("P", [40, 256, 270, 520])
@pytest.mark.parametrize("mode", ["q4", "f16"])
def test_decode_steps_with_and_without_the_shared_copy(hip, mode, P):
    host, cfg, b = batch_of(mode)
    prefix = toks(host, cfg, P, 100 + P)
    own = [16, 17, 33, 50, 20, 31, 48]
    prompts = [prefix + toks(host, cfg, n, 200 + i) for i, n in enumerate(own)]
    eligible = [True] * len(prompts)
    stranger = toks(host, cfg, P + 30, 300)                       # does not begin with the prefix
    assert stranger[:P] != prefix
    short = prefix + toks(host, cfg, 15, 301)                     # 15 ids of its own: processed whole, shares nothing
    prompts += [stranger, short]
    eligible += [False, False]
    if P == 270:                                                  # its positions cross 512 during the steps (500 + 24)
        prompts.append(prefix + toks(host, cfg, 230, 302))
        eligible.append(True)
    steps = 24

    def play(on):
        b.set_prefix(None)
        foreign_bytes(b, host, cfg, len(prompts), 900 + P)
        b.set_prefix(prefix)
        lg = prefill_all(b, list(range(len(prompts))), prompts)
        begin_streams(b, host, cfg, prompts, steps)
        ids = ragged_steps(b, prompts, 1, steps)
        last = np.stack([b.logits(q) for q in range(len(prompts))])
        chunks = [b.prefix_decode_info(q)[1] for q in range(len(prompts))]
        return lg, ids, last, chunks

    try:
        want, got = both_ways(host, play)
    finally:
        b.set_prefix(None)
    assert want[3] == [0] * len(prompts)
    assert got[3] == [P // 256 if e else 0 for e in eligible], got[3]
    assert np.array_equal(got[0], want[0]), "prompt logits"
    assert got[1] == want[1], "ids per step"
    assert np.array_equal(got[2], want[2]), ("last logits", np.nonzero((got[2] != want[2]).any(axis=1))[0].tolist())


# ---------------------------------------------------------------- 2. the serving queue


def queue_of(host, cfg, prefix, count=40):
    """the queue of tests/test_prefix_gpu.py's serve test: a quarter with their own beginnings (some short), the others behind the
    prefix, a few of those with fewer than 16 ids of their own"""
    out = []
    for j in range(count):
        if j % 4 == 3:
            out.append(toks(host, cfg, 10 + (13 * j) % 70, 700 + j))
        else:
            out.append(prefix + toks(host, cfg, 12 + (7 * j) % 45, 700 + j))
    return out


@pytest.mark.parametrize("spares", [0, -1])
@pytest.mark.parametrize("schedule", [1, 3])
def test_serve_with_and_without_the_shared_copy(hip, schedule, spares):
    host, cfg, b = batch_of("q4")
    P = 256
    prefix = toks(host, cfg, P, 510)
    queue = queue_of(host, cfg, prefix)
    eligible = sum(1 for p in queue if p[:P] == prefix and len(p) >= P + 16)
    assert 20 <= eligible < 30
    b.set_serve_schedule(schedule)
    b.set_serve_spares(spares)

    def play(on):
        b.set_prefix(prefix)
        _, _, pi0, sk0 = b.prefix_decode_info()
        ids, st = b.serve(queue, 400, -1, 8, max_new=20)
        n, _, pi1, sk1 = b.prefix_decode_info()
        assert n == P
        return ids, st, pi1 - pi0, sk1 - sk0

    try:
        want, got = both_ways(host, play)
    finally:
        b.set_prefix(None)
        b.set_serve_schedule(0)
        b.set_serve_spares(-1)
    for j in range(len(queue)):
        assert got[0][j].tolist() == want[0][j].tolist(), (schedule, spares, j)
    assert got[1]["new_tokens"] == want[1]["new_tokens"] == 20 * len(queue)
    # every prompt behind the prefix was started ONCE on a slot that shared its first chunk -- its import skipped it --, whichever
    # cache set (a sequence's own or a spare one) carried the mark there; with the switch off nobody did
    assert (want[2], want[3]) == (0, 0)
    assert got[2] == 1 and got[3] == eligible, (got[2], got[3], eligible)


# ---------------------------------------------------------------- 3. replacing the prefix while sequences decode behind it


def test_replacing_the_prefix_in_flight(hip):
    host, cfg, b = batch_of("q4")
    pa, pb = toks(host, cfg, 256, 801), toks(host, cfg, 300, 802)
    prompts = [pa + toks(host, cfg, n, 810 + i) for i, n in enumerate((16, 40, 21, 33, 18, 47))] + [toks(host, cfg, 290, 830)]
    n_sharing = 6

    def play(on):
        b.set_prefix(None)
        foreign_bytes(b, host, cfg, len(prompts), 850)
        b.set_prefix(pa)
        prefill_all(b, list(range(len(prompts))), prompts, want=False)
        begin_streams(b, host, cfg, prompts, 12)
        ids = ragged_steps(b, prompts, 1, 4)
        before = [b.prefix_decode_info(q)[1] for q in range(len(prompts))]
        imports0 = b.kv_info()[1]
        b.set_prefix(pb)                                          # the same cache set, overwritten in place
        ids += ragged_steps(b, prompts, 5, 12)
        last = np.stack([b.logits(q) for q in range(len(prompts))])
        after = [b.prefix_decode_info(q)[1] for q in range(len(prompts))]
        return ids, last, before, after, b.kv_info()[1] - imports0

    try:
        want, got = both_ways(host, play)
    finally:
        b.set_prefix(None)
    assert got[2] == [1] * n_sharing + [0] and want[2] == [0] * len(prompts)
    assert got[3] == [0] * len(prompts)
    assert got[4] == n_sharing and want[4] == 0                   # exactly those that shared went back to their own rows
    assert got[0] == want[0]
    assert np.array_equal(got[1], want[1])


# ---------------------------------------------------------------- 4. a write into a sharing sequence's prefix rows


def test_rows_rewritten_under_a_sharing_sequence(hip):
    """sequence 2's own single-sequence decoder re-decodes its rows 199 .. with other ids (as tests/test_kv_head_major_gpu.py
    does): rows inside the promised range change, the shared decoder hears of it through the watch, the sequence reads its own
    rows again -- the others go on sharing"""
    host, cfg, b = batch_of("q4")
    P = 256
    prefix = toks(host, cfg, P, 1001)
    prompts = [prefix + toks(host, cfg, n, 1010 + i) for i, n in enumerate((20, 36, 28, 44))]
    victim = 2
    L = len(prompts[victim])

    def play(on):
        b.set_prefix(None)
        foreign_bytes(b, host, cfg, len(prompts), 1050)
        b.set_prefix(prefix)
        prefill_all(b, list(range(len(prompts))), prompts, want=False)
        streams = begin_streams(b, host, cfg, prompts, 8)
        ids = ragged_steps(b, prompts, 1, 4)
        other = toks(host, cfg, L + 4, 1090)
        # steps 200 .. L + 4 of the victim alone: rows 199 .. L + 3 of another history
        b.seq_steps(victim, streams[victim][:150] + other[150:], 200, L + 4 - 199)
        chunks = [b.prefix_decode_info(q)[1] for q in range(len(prompts))]
        ids += ragged_steps(b, prompts, 5, 8)
        last = np.stack([b.logits(q) for q in range(len(prompts))])
        return ids, last, chunks

    try:
        want, got = both_ways(host, play)
    finally:
        b.set_prefix(None)
    assert got[2] == [1, 1, 0, 1] and want[2] == [0, 0, 0, 0]
    assert got[0] == want[0]
    assert np.array_equal(got[1], want[1])


# ---------------------------------------------------------------- 5. wide decoders


# 128: the nontemporal instantiation; 256: two lanes of 128 -- the shared counts are one array over all lanes
@pytest.mark.parametrize("n_seq", [128, 256])
def test_wide_decoders(hip, n_seq):
    host, cfg, b = batch_of("q4", n_seq)
    P = 256
    prefix = toks(host, cfg, P, 1201)
    # two of three sequences behind the prefix (128 is no multiple of 3: the pattern differs from lane to lane)
    prompts = [(prefix if q % 3 else toks(host, cfg, P, 1300 + q)) + toks(host, cfg, 16 + q % 23, 1500 + q) for q in range(n_seq)]
    held = [0, 1, 2, 64, 127] + ([128, 129, 130, 200, 255] if n_seq > 128 else [])

    def play(on):
        b.set_prefix(None)
        foreign_bytes(b, host, cfg, n_seq, 1250)                  # (every slot: none keeps a copy of the prefix chunk from the other side's run)
        b.set_prefix(prefix)
        prefill_all(b, list(range(n_seq)), prompts, want=False)
        begin_streams(b, host, cfg, prompts, 8)
        ids = ragged_steps(b, prompts, 1, 8, held)
        last = np.stack([b.logits(q) for q in held])
        return ids, last, [b.prefix_decode_info(q)[1] for q in range(n_seq)]

    try:
        want, got = both_ways(host, play)
    finally:
        b.set_prefix(None)
        b.close()
        del _batches[("q4", n_seq)]
    assert got[2] == [1 if q % 3 else 0 for q in range(n_seq)] and not any(want[2])
    assert got[0] == want[0]
    assert np.array_equal(got[1], want[1]), np.nonzero((got[1] != want[1]).any(axis=1))[0].tolist()


# ---------------------------------------------------------------- 6. refusals, and where nothing happens


def test_refusals_and_inert_cases(hip):
    host, cfg, b = batch_of("q4")
    P = 256
    prefix = toks(host, cfg, P, 1401)
    prompts = [prefix + toks(host, cfg, 40, 1410), toks(host, cfg, 60, 1411)]
    host.set_prefix_decode_shared(True)
    try:
        b.set_prefix(prefix)
        prefill_all(b, [0, 1], prompts, want=False)
        begin_streams(b, host, cfg, prompts, 4)
        ragged_steps(b, prompts, 1, 2)
        assert [b.prefix_decode_info(q)[1] for q in (0, 1)] == [1, 0]
        assert b.prefix_decode_share_rc(0, P + 1) != 0            # more rows than the prefix has
        assert b.prefix_decode_share_rc(1, P) != 0                # sequence 1 holds 62 rows (its next step is 63): 256 lie beyond them
        assert b.prefix_decode_share_rc(1, 63) != 0 and b.prefix_decode_share_rc(1, 62) == 0   # (62 rows: taken, and no full chunk)
        assert [b.prefix_decode_info(q)[1] for q in (0, 1)] == [1, 0]
        assert b.prefix_decode_share_rc(0, P) == 0                # the promise again: taken
        assert b.prefix_decode_share_rc(0, 0) == 0 and b.prefix_decode_info(0)[1] == 0          # ... and withdrawn
        ragged_steps(b, prompts, 3, 4)                            # (the sequence went back to its own rows)
        b.set_prefix(None)
        assert b.prefix_decode_info(0)[0] == 0
        assert b.prefix_decode_share_rc(0, 16) != 0               # no prefix set
    finally:
        b.set_prefix(None)
        host.set_prefix_decode_shared(None)
    small = host.batch(cfg, 8)                                    # 8 sequences: no shadows, no segmented prompts -- all of it is inert
    try:
        for i in range(len(cfg.weight_shapes())):
            small.set_weight(i, host.synth_weight(cfg, 777, i))
        assert small.set_prefix_rc(prefix) == -2
        assert small.prefix_decode_share_rc(0, 256) == 0
        assert small.prefix_decode_info(0) == (0, 0, 0, 0)
    finally:
        small.close()
