"""-m gpu: n samples per prompt (include/gten_host_samples.h, include/gten_hip_groups.h).  serve_samples processes
a group's prompt once and lets its members' decode slots read the prompt's full chunks from one group record of the decoder.  The
contract is an equality: ids, ended_by, log-prob records and totals are, byte for byte, those of the EXISTING queue with all six
stages (serve_fsm with n_top) on the expanded prompts -- every prompt written out n times in a row -- with nothing registered and
gten_hip_set_prefix_decode_shared(0).  That run is the reference of every comparison here."""
import numpy as np
import pytest

from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from helpers import F16, Q4, Q8, tiny_config
from test_model_gpu import host_cfg
from test_prefix_decode_gpu import begin_streams, foreign_bytes, prefill_all, toks
import samples_ref

pytestmark = pytest.mark.gpu

MAX_CTX = 768                 # three chunks of 256 positions
SEED = 20241020
NEW = 12                      # new ids per item
GROUPS = 64                   # GTEN_GROUPS_MAX: the records are off by default (set_groups_cap(-1) is 0), the tests switch them on
_batches = {}
_refs = {}


def new_batch(mode, n_seq=16):
    """2 layers, 4 heads / 2 kv heads, d_head 64 (the model of tests/test_prefixes_gpu.py), with a stop automaton in the pool: every
    third id of the vocabulary ends a bound sequence"""
    wd, ad = {"q4": (Q4, Q8), "f16": (F16, F16)}[mode]
    pkg = load_package()
    host = pkg.load_host()
    cfg = host_cfg(tiny_config(wd, ad, n_heads=4, n_kv_heads=2, n_layers=2, max_ctx=MAX_CTX))
    b = host.batch(cfg, n_seq)
    for i in range(len(cfg.weight_shapes())):
        b.set_weight(i, host.synth_weight(cfg, 777, i))
    f = pkg.hostabi.Fsm(host, cfg.n_vocab)
    b.stop_start = f.add_stop([[i] for i in range(0, cfg.n_vocab, 3)])
    b.set_fsm(f)
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
    _refs.clear()


def expanded(v, ns):
    return v if np.isscalar(v) else samples_ref.expand(list(v), ns)


def reference(host, b, prompts, ns, top_k=40, temp=0.9, fsm_start=-1, slice_steps=8):
    """the existing queue on the expanded prompts, nothing registered, every sequence on its own copy: (ids, stats, ended_by, records)"""
    host.set_prefix_decode_shared(False)
    try:
        return b.serve_fsm(samples_ref.expand(prompts, ns), MAX_CTX, -1, expanded(top_k, ns), expanded(temp, ns), SEED, expanded(fsm_start, ns),
                           slice_steps=slice_steps, max_new=NEW, n_top=3)
    finally:
        host.set_prefix_decode_shared(None)


def samples(b, prompts, ns, top_k=40, temp=0.9, fsm_start=-1, slice_steps=8):
    return b.serve_samples_items(prompts, ns, MAX_CTX, -1, top_k, temp, SEED, fsm_start=fsm_start, slice_steps=slice_steps, max_new=NEW, n_top=3)


def assert_same(got, want, what=""):
    assert len(got[0]) == len(want[0])
    for e in range(len(want[0])):
        assert np.array_equal(got[0][e], want[0][e]), (what, "ids of item", e)
    assert np.array_equal(got[2], want[2]), (what, "ended_by")
    for k, name in ((3, "logprob"), (4, "top_id"), (5, "top_logprob")):
        assert np.array_equal(got[k], want[k]), (what, name, np.nonzero((got[k] != want[k]).reshape(len(want[0]), -1).any(axis=1))[0].tolist())


def info_delta(b, before):
    return tuple(a - c for a, c in zip(b.samples_info(), before))


# ---------------------------------------------------------------- 1. the queue

LENS = [15, 16, 40, 255, 256, 257, 300, 520]      # 15: processed whole, one by one; 255 / 256 / 257: around one chunk; 520: two chunks
NS = [1, 1, 1, 2, 2, 3, 1, 5]                     # 16 items: every group fits the 16 sets whatever the schedule, so no group is cut
GREEDY, STOPPED = 5, 3                            # the 257-id prompt is greedy (its samples are equal), the 255-id one is bound to the stop


def queue_prompts(host, cfg):
    return [toks(host, cfg, n, 3100 + n) for n in LENS]


@pytest.mark.parametrize("spares", [0, 4])
@pytest.mark.parametrize("schedule", [1, 3])
@pytest.mark.parametrize("mode", ["q4", "f16"])
def test_queue_of_sample_groups(hip, mode, schedule, spares):
    host, cfg, b = batch_of(mode)
    prompts = queue_prompts(host, cfg)
    top_k = [0 if j == GREEDY else 40 for j in range(len(LENS))]
    start = [b.stop_start if j == STOPPED else -1 for j in range(len(LENS))]
    if mode not in _refs:                                         # (one reference per configuration: the ids do not depend on the schedule)
        _refs[mode] = reference(host, b, prompts, NS, top_k, 0.9, start)
    want = _refs[mode]
    b.set_serve_schedule(schedule)
    b.set_serve_spares(spares)
    b.set_groups_cap(GROUPS)
    try:
        before = b.samples_info()
        skipped = b.prefix_decode_info(0)[3]
        got = samples(b, prompts, NS, top_k, 0.9, start)
        delta = info_delta(b, before)
        skipped = b.prefix_decode_info(0)[3] - skipped
    finally:
        b.set_serve_schedule(0)
        b.set_serve_spares(-1)
        b.set_groups_cap(-1)
    assert_same(got, want, (mode, schedule, spares))
    first = samples_ref.first_items(NS)
    assert sum(NS) == 16 and got[1]["admissions"] == want[1]["admissions"] == 16 and got[1]["new_tokens"] == want[1]["new_tokens"]
    g = samples_ref.regroup(got[0], NS)[GREEDY]
    assert all(np.array_equal(s, g[0]) for s in g) and len(g[0]) == LENS[GREEDY] + NEW        # greedy: all its samples equal
    s = samples_ref.regroup(got[0], NS)[6]
    assert len(s[0]) == LENS[6] + NEW
    five = samples_ref.regroup(got[0], NS)[7]
    assert len({tuple(x.tolist()) for x in five}) > 1                                         # sampled with other streams: they differ
    ended = got[2][first[STOPPED]: first[STOPPED + 1]]
    assert 2 in ended.tolist()                                    # (a third of the vocabulary stops it: (2/3)^24 that neither sample ends)
    # exactly the copies of the batched prompts, and exactly their rows: the 15-id prompt is no segment, n = 1 has no copy
    copies = sum(n - 1 for p, n in zip(LENS, NS) if p >= 16)
    rows = sum((n - 1) * p for p, n in zip(LENS, NS) if p >= 16)
    assert delta[0] == copies == 8 and delta[1] == rows
    # the groups behind a full chunk (256, 257, 520) each got a record, the 255-id group carries no mark; none is left
    assert delta[2:] == (3, 0, 0) and b.samples_info()[4] == 0
    assert skipped >= 2 + 3 + 5                                   # every member's import left the chunks of its record out
    assert got[1]["prefill_s"] > 0


# ---------------------------------------------------------------- 2. records are read


def positions(prompts, n_seq, t):
    return [len(p) + t for p in prompts] + [t] * (n_seq - len(prompts))


def step_all(b, ns, held, graph):
    b.decode_step_ragged(ns, use_graph=graph)
    return [b.decode_result(q, ns[q]) for q in held]


@pytest.mark.parametrize("mode", ["q4", "f16"])
def test_members_read_their_chunks_from_a_record(hip, mode):
    host, cfg, b = batch_of(mode)
    plan = [(256, 3), (257, 10), (520, 63), (255, 0)]            # (prompt ids, group record)
    prompts, groups = [], []
    for P, g in plan:
        p = toks(host, cfg, P, 3300 + P)
        groups.append((g, P, list(range(len(prompts), len(prompts) + 3))))
        prompts += [p, p, p]
    steps = 6

    def play(on):
        foreign_bytes(b, host, cfg, len(prompts), 3350)
        prefill_all(b, list(range(len(prompts))), prompts, want=False)
        skipped = b.prefix_decode_info(0)[3]
        if on:
            for g, P, seqs in groups:
                assert b.group_decode_set_rc(g, seqs[0], P) == 0
                for q in seqs:
                    assert b.group_decode_share_rc(q, g, P) == 0
        begin_streams(b, host, cfg, prompts, steps)
        held = list(range(len(prompts)))
        ids = [step_all(b, positions(prompts, b.n_seq, t), held, t % 2 == 0) for t in (1, 2)]
        views = [b.groups_decode_info(q) for q in held]
        pviews = [b.prefix_decode_info_at(q) for q in held]
        ids += [step_all(b, positions(prompts, b.n_seq, t), held, t % 2 == 0) for t in range(3, steps + 1)]
        last = np.stack([b.logits(q) for q in held])
        rec = [b.groups_decode_info(0, g)[2:] for g, _, _ in groups]
        if on:
            for g, _, _ in groups:
                assert b.group_decode_set_rc(g, None) == 0
        return ids, last, views, pviews, b.prefix_decode_info(0)[3] - skipped, rec

    host.set_prefix_decode_shared(False)
    try:
        want = play(False)
    finally:
        host.set_prefix_decode_shared(None)
    base = [b.groups_decode_info(0, g)[3] for g, _, _ in groups]
    got = play(True)
    assert want[2] == [(-1, 0)] * 12 and want[4] == 0
    assert got[2] == [(3, 1)] * 3 + [(10, 1)] * 3 + [(63, 2)] * 3 + [(-1, 0)] * 3, got[2]     # 1 / 1 / 2 chunks; behind 255 ids none
    assert got[3] == [(-1, 0)] * 12                               # a sequence on a group record reports "no prefix"
    assert got[4] == 9                                            # the imports of the nine sharers skipped their shared chunks
    assert got[5] == [(256, base[0] + 1, 3), (257, base[1] + 1, 3), (520, base[2] + 1, 3), (255, base[3] + 1, 0)]
    assert got[0] == want[0], "ids per step"
    assert np.array_equal(got[1], want[1]), "last logits"


# ---------------------------------------------------------------- 3. the snapshot


def test_record_is_a_snapshot_of_the_rows_it_was_taken_from(hip):
    """four members behind 300 ids, record 7 taken from sequence 0's set.  After one step that set is overwritten with another prompt
    through the library: sequence 0 comes off (its rows were written), the siblings keep their chunks, nothing but sequence 0 is
    imported again and the record's shadow is not imported a second time"""
    host, cfg, b = batch_of("q4")
    P, G = 300, 7
    p = toks(host, cfg, P, 3401)
    other = toks(host, cfg, P + 1, 3402)                          # (one id more: its first step is the step the siblings take, so the
                                                                  #  run continues for everybody and nobody is restarted)
    prompts = [p, p, p, p]
    steps = 6

    def play(on):
        foreign_bytes(b, host, cfg, 4, 3450)
        prefill_all(b, [0, 1, 2, 3], prompts, want=False)
        if on:
            assert b.group_decode_set_rc(G, 0, P) == 0
            for q in range(4):
                assert b.group_decode_share_rc(q, G, P) == 0
        begin_streams(b, host, cfg, prompts, steps)
        ids = [step_all(b, positions(prompts, b.n_seq, 1), [0, 1, 2, 3], False)]
        before = [b.groups_decode_info(q, G) for q in range(4)]
        imports0 = b.kv_info()[1]
        b.prefill(0, other, want=False)                           # another prompt onto the set the record was taken from
        b.decode_begin(0, other + toks(host, cfg, steps, 3403))
        after = [b.groups_decode_info(q, G) for q in range(4)]
        for t in range(2, steps + 1):
            ns = positions(prompts, b.n_seq, t)
            ns[0] = len(other) + t - 1
            ids.append(step_all(b, ns, [0, 1, 2, 3], t % 2 == 0))
        end = [b.groups_decode_info(q, G) for q in range(4)]
        last = np.stack([b.logits(q) for q in range(4)])
        if on:
            assert b.group_decode_set_rc(G, None) == 0
        return ids, last, before, after, end, b.kv_info()[1] - imports0

    host.set_prefix_decode_shared(False)
    try:
        want = play(False)
    finally:
        host.set_prefix_decode_shared(None)
    base = b.groups_decode_info(0, G)[3]
    got = play(True)
    assert got[2] == [(G, 1, P, base + 1, 4)] * 4
    assert got[3] == got[4] == [(-1, 0, P, base + 1, 3)] + [(G, 1, P, base + 1, 3)] * 3      # the siblings keep sharers and chunks
    assert got[5] == want[5] == 1                                 # sequence 0's own rows, and no full import of a sibling
    assert got[0] == want[0], "ids per step"
    assert np.array_equal(got[1], want[1])


# ---------------------------------------------------------------- 4. a group behind a registered prefix


def test_group_behind_a_registered_prefix(hip):
    host, cfg, b = batch_of("q4")
    prefix = toks(host, cfg, 256, 3501)
    prompts = [toks(host, cfg, 70, 3502), prefix + toks(host, cfg, 44, 3503), toks(host, cfg, 280, 3504)]
    ns = [1, 3, 2]
    want = reference(host, b, prompts, ns)
    b.set_prefix_at(0, prefix)
    b.set_groups_cap(GROUPS)
    try:
        before, pre = b.samples_info(), b.prefixes_info(0)
        shadow = b.prefix_decode_info_at(0, 0)[3]
        got = samples(b, prompts, ns)
        delta, post = info_delta(b, before), b.prefixes_info(0)
        shadow = b.prefix_decode_info_at(0, 0)[3] - shadow
    finally:
        b.set_prefix_at(0, None)
        b.set_groups_cap(-1)
    assert_same(got, want)
    assert post[1] - pre[1] == 1 and post[2] - pre[2] == 44       # the leader took the short way: 44 rows, once
    assert delta[0] == 3 and delta[1] == 2 * 44 + 280             # (a copy behind the prefix would have cost its own rows only)
    assert delta[2:] == (2, 0, 0)                                 # both groups read from group records ...
    assert shadow == 0                                            # ... and nobody from the prefix's shadow: it was never imported


# ---------------------------------------------------------------- 5. the pool of records exhausted, a group larger than the sets


def test_record_pool_exhausted_and_group_cut(hip):
    host, cfg, b = batch_of("q4")
    prompts = [toks(host, cfg, 300, 3601), toks(host, cfg, 400, 3602)]
    ns = [3, 3]
    want = reference(host, b, prompts, ns)
    try:
        # (cap 1: the second group decodes unshared; 0 and the default, which is 0: nothing is shared; 64, and 1000 clamped to it: both)
        for cap, expect in ((1, (4, 700 * 2, 1, 1, 0)), (0, (4, 700 * 2, 0, 2, 0)), (-1, (4, 700 * 2, 0, 2, 0)), (GROUPS, (4, 700 * 2, 2, 0, 0)),
                            (1000, (4, 700 * 2, 2, 0, 0))):
            b.set_groups_cap(cap)
            before = b.samples_info()
            got = samples(b, prompts, ns)
            assert info_delta(b, before) == expect, (cap, info_delta(b, before))
            assert_same(got, want, cap)
    finally:
        b.set_groups_cap(-1)
    # 20 samples on 16 slots without spares: 16 members share the first prompt pass; they end together (no eos, equal budgets),
    # and the four that are left are a later group with a pass of its own
    # (a batch of its own: the module's has kept the spare sets of earlier queues, and a queue takes every set there is)
    one = [toks(host, cfg, 300, 3603)]
    _, _, b = new_batch("q4")
    try:
        b.set_serve_spares(0)
        b.set_groups_cap(GROUPS)
        want = reference(host, b, one, [20])
        before = b.samples_info()
        got = samples(b, one, [20])
        delta = info_delta(b, before)
    finally:
        b.close()
    assert_same(got, want, "cut")
    assert got[1]["admissions"] == 20 and delta[0] == 15 + 3 and delta[1] == 18 * 300 and delta[2:] == (2, 0, 0)


# ---------------------------------------------------------------- 6. width


def test_queue_on_128_slots(hip):
    host, cfg, b = new_batch("q4", 128)
    try:
        prompts = [toks(host, cfg, 256 + (37 * j) % 265, 3700 + j) for j in range(36)]        # 256 .. 520 ids
        ns = [4] * 36                                             # 144 items through 128 slots and 32 spares
        want = reference(host, b, prompts, ns, slice_steps=4)
        b.set_groups_cap(GROUPS)
        before = b.samples_info()
        got = samples(b, prompts, ns, slice_steps=4)
        delta = info_delta(b, before)
    finally:
        b.close()
    assert_same(got, want)
    assert got[1]["admissions"] == 144 and got[1]["new_tokens"] == want[1]["new_tokens"] == 144 * NEW
    # 144 items on 160 cache sets: no group is cut; at most 36 groups in flight: a record was always free
    assert delta == (36 * 3, 3 * sum(len(p) for p in prompts), 36, 0, 0), delta


# ---------------------------------------------------------------- 7. a small batch: correct, nothing copied


def test_small_batch_runs_every_member_as_an_ordinary_item(hip):
    host, cfg, b = new_batch("q4", 8)
    try:
        prompts = [toks(host, cfg, n, 3800 + n) for n in (40, 300)]
        ns = [3, 2]
        want = reference(host, b, prompts, ns)
        before = b.samples_info()
        got = samples(b, prompts, ns)
        assert info_delta(b, before) == (0, 0, 0, 0, 0)
        assert b.group_decode_set_rc(0, 0, 16) == 0 and b.group_decode_share_rc(0, 0, 16) == 0 and b.groups_decode_info(0, 0) == (-1, 0, 0, 0, 0)
        # the public call: per prompt its samples; best_of keeps the first k by samples_rank
        grouped = b.serve_samples(prompts, ns, MAX_CTX, -1, 40, 0.9, SEED, n_top=3, slice_steps=8, max_new=NEW)
        best = b.serve_samples(prompts, ns, MAX_CTX, -1, 40, 0.9, SEED, best_of=1, slice_steps=8, max_new=NEW)
    finally:
        b.close()
    assert_same(got, want)
    first = samples_ref.first_items(ns)
    for j in range(2):
        assert [s.tolist() for s in grouped[0][j]] == [got[0][e].tolist() for e in range(first[j], first[j + 1])]
        assert np.array_equal(grouped[3][j], got[3][first[j]: first[j + 1]]) and np.array_equal(grouped[2][j], got[2][first[j]: first[j + 1]])
        n_new = [len(got[0][e]) - len(prompts[j]) for e in range(first[j], first[j + 1])]
        order = samples_ref.rank(samples_ref.record_sums(got[3][first[j]: first[j + 1]], len(prompts[j]), n_new), n_new)
        assert len(best) == 3 and len(best[0][j]) == 1 and best[0][j][0].tolist() == got[0][first[j] + order[0]].tolist()


# ---------------------------------------------------------------- 8. the device calls alone


def test_device_calls_refusals_and_release(hip):
    host, cfg, b = batch_of("q4")
    api = load_package().hipabi.load()
    dec = b.fsm_decoder()
    p = toks(host, cfg, 300, 3901)
    prompts = [p, p, p, toks(host, cfg, 60, 3902)]
    host.set_prefix_decode_shared(True)
    try:
        foreign_bytes(b, host, cfg, 4, 3950)
        prefill_all(b, [0, 1, 2, 3], prompts, want=False)
        begin_streams(b, host, cfg, prompts, 4)
        step_all(b, positions(prompts, b.n_seq, 1), [0], False)
        base = b.groups_decode_info(0, 5)[3]
        assert b.group_decode_set_rc(-1, 0, 300) != 0 and b.group_decode_set_rc(64, 0, 300) != 0     # record outside [0, 64)
        assert api.decoder_group_set(dec, 64, None, 0) != 0
        assert api.decoder_group_share(dec, 0, -1, 256) != 0 and api.decoder_group_share(dec, 0, 64, 256) != 0
        assert api.decoder_group_share(dec, 0, 5, 256) != 0                                          # record 5 is not set
        assert b.group_decode_set_rc(5, 0, 300) == 0
        assert api.decoder_groups_info(dec, 0, 5) == (-1, 0, 300, base + 1, 0)
        assert api.decoder_group_share(dec, 1, 5, 301) != 0                                          # rows beyond the record
        assert api.decoder_group_share(dec, 3, 5, 256) != 0                                          # sequence 3 holds 61 rows
        assert api.decoder_group_share(dec, 3, 5, 60) == 0 and b.groups_decode_info(3) == (-1, 0)    # (60 rows: taken, no full chunk)
        assert [b.groups_decode_info(q) for q in range(3)] == [(-1, 0)] * 3                          # refusals record nothing
        for q in range(3):
            assert api.decoder_group_share(dec, q, 5, 300) == 0
        assert [b.groups_decode_info(q) for q in range(3)] == [(5, 1)] * 3 and b.groups_decode_info(0, 5)[4] == 3
        assert api.decoder_group_share(dec, 2, 5, 0) == 0 and b.groups_decode_info(2) == (-1, 0)     # withdrawn
        assert api.decoder_group_share(dec, 2, 5, 300) == 0
        step_all(b, positions(prompts, b.n_seq, 2), [0], True)
        imports = b.kv_info()[1]
        assert api.decoder_group_set(dec, 5, None, 0) == 0                                           # release: the sharers come off ...
        assert [b.groups_decode_info(q) for q in range(3)] == [(-1, 0)] * 3
        assert b.groups_decode_info(0, 5)[2:] == (0, base + 1, 0)
        assert api.decoder_group_share(dec, 0, 5, 256) != 0
        step_all(b, positions(prompts, b.n_seq, 3), [0], False)
        assert b.kv_info()[1] - imports == 3                                                         # ... and import their own rows
    finally:
        b.group_decode_set_rc(5, None)
        host.set_prefix_decode_shared(None)


def test_first_group_on_a_decoder_that_used_only_a_prefix(hip):
    """a FRESH decoder takes steps sharing prefix 0 only (the one-prefix attention), then its first group record is set mid-run
    (the step changes to the instantiations that pick a shadow from the table, the graphs captured so far go): same ids"""
    host, cfg, ref = batch_of("q4")
    F, S = toks(host, cfg, 256, 4001), toks(host, cfg, 270, 4002)
    prompts = [F + toks(host, cfg, n, 4010 + i) for i, n in enumerate((16, 29))] + [S, S, S] + [toks(host, cfg, 280, 4020)]
    steps = 10

    def play(b, on):
        foreign_bytes(b, host, cfg, len(prompts), 4050)
        if on:
            b.set_prefix_at(0, F)
        prefill_all(b, list(range(len(prompts))), prompts, want=False)
        begin_streams(b, host, cfg, prompts, steps)
        held = list(range(len(prompts)))
        ids = [step_all(b, positions(prompts, b.n_seq, t), held, t % 2 == 0) for t in range(1, 6)]
        before = [(b.prefix_decode_info_at(q), b.groups_decode_info(q)) for q in held]
        if on:
            assert b.group_decode_set_rc(40, 2, len(S)) == 0
            for q in (2, 3, 4):
                assert b.group_decode_share_rc(q, 40, len(S)) == 0
        ids += [step_all(b, positions(prompts, b.n_seq, t), held, t % 2 == 0) for t in range(6, steps + 1)]
        after = [(b.prefix_decode_info_at(q), b.groups_decode_info(q)) for q in held]
        return ids, np.stack([b.logits(q) for q in held]), before, after

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
    none = ((-1, 0), (-1, 0))
    assert got[2] == [((0, 1), (-1, 0))] * 2 + [none] * 4
    assert got[3] == [((0, 1), (-1, 0))] * 2 + [((-1, 0), (40, 1))] * 3 + [none]               # the prefix's sharers stay on it
    assert got[0] == want[0]
    assert np.array_equal(got[1], want[1])
