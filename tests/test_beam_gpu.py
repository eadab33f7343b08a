"""-m gpu: beam search on the device (include/gten_hip_beam.h, include/gten_host_beam.h).

The round is held to tests/beam_ref.py byte for byte on constructed lists; the in-place gather to numpy with guard bytes; the whole
search to beam_ref's search over lists that no beam code produced (the prompt prefilled on one sequence, the prefix teacher-forced
step by step, gten_hip_row_top_logprobs on each step's logits): ids, final, cum and ended_by bit for bit."""
import numpy as np
import pytest

import beam_ref as ref
from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from helpers import F16, Q4, Q8, tiny_config
from test_model_gpu import host_cfg

pytestmark = pytest.mark.gpu

EOS = 7
STRIDE = 16                          # list row stride: 2 * GTEN_HIP_BEAM_MAX
ROUNDS = 5


def dev(hip, a):
    return load_package().hipabi.DeviceBuffer.from_numpy(hip, np.ascontiguousarray(a))


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ the round

def lists_of(kind, B, t, cum, rng):
    """the lists of one group's B rows for round t: (top_id[B][16], top_lp[B][16]), every row in descending order"""
    L = 2 * B
    ti = np.zeros((B, STRIDE), np.int32)
    tl = np.zeros((B, STRIDE), np.float32)
    for b in range(B):
        ids = rng.choice(np.arange(8, 512), L, replace=False)
        if kind == "ties":
            lp = -np.sort(rng.integers(0, 4, L)).astype(np.float32) * 0.5           # a grid: equal scores inside a beam and across beams
        else:
            lp = -np.sort(rng.random(L).astype(np.float32) * 4.0)
        if kind in ("mixed", "ties", "noeos") and rng.random() < 0.6:
            ids[rng.integers(0, L)] = EOS
        ti[b, :L], tl[b, :L] = ids, lp
    far = -30.0 - np.arange(L, dtype=np.float32)
    if kind in ("eos0", "eosB1") and t == 1:
        ti[0, 0 if kind == "eos0" else B - 1] = EOS                               # round 1 has one source: its list rank is the walk's rank
    if kind == "eosB" and t == 1:
        tl[0, :L] = -1.0 - 0.15 * np.arange(L, dtype=np.float32)
    if kind == "eosB" and t == 2 and B >= 2:
        # eos of beam 0 at rank 0, B - 1 others of beam 0, then the eos of beam 1 at rank B: dropped
        for b in range(B):
            tl[b, :L] = far
            ti[b, 0], tl[b, 0] = EOS, -0.1
        tl[0, 1:B] = -0.1 - 0.001 * np.arange(1, B, dtype=np.float32)
        tl[1, 1:L] = -0.2 - 0.001 * np.arange(1, L, dtype=np.float32)
    if kind in ("replace", "noreplace"):
        if t == 1:                                                                # B = 3: one finishes at rank 2 (replace) or 1
            tl[0, :L] = [-1, -2, -9, -10, -11, -12] if kind == "replace" else [-1, -2, -3, -4, -5, -6]
            ti[0, 2 if kind == "replace" else 1] = EOS
        if t == 2:                                                                # every beam's eos in the first B ranks: a fourth record
            for b in range(B):
                tl[b, :L] = far
                ti[b, 0], tl[b, 0] = EOS, -0.1
    return ti, tl


CASES = [[(1, "plain")]] + [[(B, "mixed")] for B in (1, 2, 3, 8)] + [[(B, "ties")] for B in (2, 8)] + [
    [(3, "replace"), (3, "noreplace"), (8, "ties"), (1, "eosB1"), (2, "noeos")],
    [(2, "eos0"), (8, "eosB"), (3, "ties"), (1, "mixed"), (3, "eosB1")],
    [(2, "eosB"), (1, "eos0"), (8, "mixed"), (3, "mixed"), (8, "eos0")]]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_round_equals_the_restatement_byte_for_byte(hip, case):
    groups = CASES[case]
    G = len(groups)
    rng = np.random.default_rng(100 + case)
    max_new = ROUNDS - 1 if groups[0][1] == "plain" else ROUNDS + 2    # (plain: the fifth call finds the group out of rounds)
    rows = ROUNDS + 3
    w = ref.weights(rows, 0.9)
    row0 = np.cumsum([0] + [B for B, _ in groups])
    n_rows = int(row0[-1])
    garr = np.array([(int(row0[g]), B, 0, max_new, -1 if kind == "noeos" else EOS) for g, (B, kind) in enumerate(groups)], dtype=hip.BEAM_GROUP)
    states = [ref.new_state() for _ in range(G)]
    trel_p, trel_i = np.zeros((G, rows, 8), np.int32), np.zeros((G, rows, 8), np.int32)
    nxt = np.full(n_rows, -5, np.int32)
    d_groups, d_state, d_w = dev(hip, garr), dev(hip, np.zeros(G, hip.BEAM_STATE)), dev(hip, w)
    d_par, d_ids, d_next = dev(hip, trel_p), dev(hip, trel_i), dev(hip, nxt)
    trace = {g: [] for g in range(G)}
    frozen = 0
    for t in range(1, ROUNDS + 1):
        ti, tl = np.zeros((n_rows, STRIDE), np.int32), np.full((n_rows, STRIDE), np.float32(3e38))
        for g, (B, kind) in enumerate(groups):
            a, b = lists_of(kind, B, t, states[g]["cum"], rng)
            ti[row0[g]: row0[g + 1]], tl[row0[g]: row0[g + 1]] = a, b
            before = states[g].tobytes()
            got = ref.round_(states[g], a, b, B, int(garr["eos"][g]), w, max_new, trace[g])
            if got is None:
                frozen += states[g]["done"] != 0
                assert states[g]["done"] == 0 or states[g].tobytes() == before
                continue
            trel_p[g, t], trel_i[g, t] = got[0], got[1]
            nxt[row0[g]: row0[g + 1]] = got[2]
        d_ti, d_tl = dev(hip, ti), dev(hip, tl)
        hip.beam_round(d_groups, d_state, d_ti, d_tl, STRIDE, d_w, len(w), d_par, d_ids, rows, d_next)
        hip.sync()
        st = d_state.download(np.uint8).reshape(G, 176)
        for g in range(G):
            assert st[g].tobytes() == states[g].tobytes(), (case, t, g, np.frombuffer(st[g].tobytes(), hip.BEAM_STATE), states[g])
        assert (d_par.download(np.int32).reshape(G, rows, 8) == trel_p).all(), (case, t)
        assert (d_ids.download(np.int32).reshape(G, rows, 8) == trel_i).all(), (case, t)
        assert d_next.download(np.int32).tolist() == nxt.tolist(), (case, t)
    ev = {kind: trace[g] for g, (_, kind) in enumerate(groups)}
    if groups[0][1] == "plain":
        assert states[0]["t"] == ROUNDS - 1 and states[0]["stepped"] == 0
    if "replace" in ev:
        assert ev["replace"] == ["finish", "finish", "finish", "replace"] and ev["noreplace"] == ["finish", "finish", "finish", "keep"]
        assert frozen >= 6                                             # two done groups stood still for three rounds beside live ones
    if "eosB1" in ev and "eos0" in ev:
        assert ev["eos0"][0] == "finish" and "drop" in ev["eosB"] and ev["eosB1"][0] == "finish"
    if "noeos" in ev:
        assert ev["noeos"] == []


def test_round_leaves_a_group_whose_lists_would_overlap_alone(hip):
    """row_stride below 2 * n_beams: the group is not advanced (not one byte of it changes), its neighbour is"""
    garr = np.array([(0, 2, 0, 4, -1), (2, 1, 0, 4, -1)], dtype=hip.BEAM_GROUP)
    ti = np.arange(8, 8 + 3 * 3, dtype=np.int32).reshape(3, 3)
    tl = -np.arange(9, dtype=np.float32).reshape(3, 3)
    w = ref.weights(4, 1.0)
    bufs = [dev(hip, garr), dev(hip, np.zeros(2, hip.BEAM_STATE)), dev(hip, ti), dev(hip, tl), dev(hip, w), dev(hip, np.zeros((2, 5, 8), np.int32)),
            dev(hip, np.zeros((2, 5, 8), np.int32)), dev(hip, np.full(3, -5, np.int32))]
    hip.beam_round(bufs[0], bufs[1], bufs[2], bufs[3], 3, bufs[4], len(w), bufs[5], bufs[6], 5, bufs[7])
    hip.sync()
    st = np.frombuffer(bufs[1].download(np.uint8).tobytes(), hip.BEAM_STATE)
    assert st[0].tobytes() == bytes(176) and st[1]["t"] == 1 and st[1]["stepped"] == 1
    assert bufs[7].download(np.int32).tolist() == [-5, -5, int(ti[2, 0])]


# ------------------------------------------------------------------------------------------------------------ the gather

GUARD = 64
ROT = [1, 2, 3, 4, 5, 6, 7, 0]


def run_permute(hip, parents, Bs, offset, nbytes, n_ranges=2, done=None, base_shift=0):
    """group g (Bs[g] sets, parents[g]) gets n_ranges ranges; every set is GUARD + offset + nbytes + GUARD bytes of random data.  Checks
    the whole buffer -- guards and the bytes in front of `offset` included -- against numpy."""
    rng = np.random.default_rng(nbytes + offset)
    G = len(Bs)
    span = GUARD + base_shift + offset + nbytes + GUARD
    span = (span + 255) // 256 * 256
    layout, n_sets = [], 0
    for g in range(G):
        for _ in range(n_ranges):
            layout.append((g, [n_sets + b for b in range(Bs[g])]))
            n_sets += Bs[g]
    data = rng.integers(0, 256, (n_sets, span), dtype=np.uint8)
    buf = dev(hip, data)
    want = data.copy()
    lo = GUARD + base_shift + offset
    for g, sets in layout:
        if done is not None and done[g]:
            continue
        for b, s in enumerate(sets):
            want[s, lo: lo + nbytes] = data[sets[parents[g][b]], lo: lo + nbytes]
    garr = np.array([(0, Bs[g], 0, 4, -1) for g in range(G)], dtype=hip.BEAM_GROUP)
    ranges = [(g, [buf.ptr + s * span + GUARD + base_shift for s in sets]) for g, sets in layout]
    par = np.zeros((G, 8), np.int32)
    for g in range(G):
        par[g, : Bs[g]] = parents[g]
    d_groups = dev(hip, garr)                                          # (alive until the launch has run)
    if done is None:
        d_par = dev(hip, par)
        hip.permute_sets(ranges, offset, nbytes, d_groups.ptr, G, None, d_par.ptr)
    else:
        st = np.zeros(G, hip.BEAM_STATE)
        st["t"], st["stepped"], st["done"] = 2, 1, done
        trel = np.full((G, 4, 8), 99, np.int32)                        # (rows other than t hold parents outside every group: never read)
        trel[:, 2] = par
        d_state, d_par = dev(hip, st), dev(hip, trel)
        hip.permute_sets(ranges, offset, nbytes, d_groups.ptr, G, d_state.ptr, d_par.ptr, 4)
    hip.sync()
    got = buf.download(np.uint8).reshape(n_sets, span)
    assert (got == want).all(), (parents, offset, nbytes, np.argwhere(got != want)[:4])


@pytest.mark.parametrize("nbytes", [4, 68, 136 * 3, 272 * 5, 512 * 7, 4080, 4112, 1020, 1028])
def test_permute_sets_in_place_against_numpy(hip, nbytes):
    mix = [0, 0, 2, 7, 4, 2, 6, 3]                                     # fixed points 0, 2, 4, 6; 2 read twice; 7 and 3 moved
    for offset in ((0, 32, 4, 72) if nbytes in (4, 68, 408, 1360, 3584) else (0, 4)):
        run_permute(hip, [list(range(8))], [8], offset, nbytes)       # the identity: nothing written
        run_permute(hip, [ROT], [8], offset, nbytes)                  # a full rotation: every set is source and destination
        run_permute(hip, [[5] * 8], [8], offset, nbytes)              # all from one set
        run_permute(hip, [mix], [8], offset, nbytes)
        run_permute(hip, [[1, 0], [2, 0, 1], [0]], [2, 3, 1], offset, nbytes, n_ranges=3)      # a swap, a 3-cycle, one beam
    run_permute(hip, [ROT], [8], 0, nbytes, base_shift=4)             # bases that are 4- but not 16-byte aligned
    # two groups with different parents in one launch, one of them done; then the other one
    run_permute(hip, [[2, 2, 0], [1, 0, 0, 3]], [3, 4], 16, nbytes, done=[0, 1])
    run_permute(hip, [[2, 2, 0], [1, 0, 0, 3]], [3, 4], 16, nbytes, done=[1, 0])
    run_permute(hip, [[2, 2, 0], [1, 0, 0, 3]], [3, 4], 20, nbytes, done=[0, 0])


def test_permute_sets_refusals(hip):
    buf = dev(hip, np.zeros(1024, np.uint8))
    g = dev(hip, np.array([(0, 2, 0, 4, -1)], dtype=hip.BEAM_GROUP))
    par = dev(hip, np.zeros(8, np.int32))
    ok = [(0, [buf.ptr, buf.ptr + 512])]
    assert hip.permute_sets_rc(ok, 0, 64, g.ptr, 1, None, par.ptr) == 0
    assert hip.permute_sets_rc(ok, 0, 0, g.ptr, 1, None, par.ptr) == 0
    hip.sync()
    assert hip.permute_sets_rc(ok, 0, 66, g.ptr, 1, None, par.ptr) != 0 and "multiples of 4" in hip.last_error()
    assert hip.permute_sets_rc(ok, 2, 64, g.ptr, 1, None, par.ptr) != 0
    assert hip.permute_sets_rc([(0, [buf.ptr + 2, buf.ptr + 512])], 0, 64, g.ptr, 1, None, par.ptr) != 0 and "aligned" in hip.last_error()
    assert hip.permute_sets_rc([(1, [buf.ptr, buf.ptr + 512])], 0, 64, g.ptr, 1, None, par.ptr) != 0
    assert hip.permute_sets_rc([], 0, 64, g.ptr, 1, None, par.ptr) != 0


# ------------------------------------------------------------------------------------------------------------ the whole search

MODES = {"q4": (Q4, Q8), "q8": (Q8, Q8), "f16": (F16, F16)}
MAX_NEW = 6
_models = {}


def batch_of(mode, n_seq, max_ctx=64):
    """one batch per (mode, width) for the whole module: synthetic weights, the tiny model"""
    key = (mode, n_seq)
    if key not in _models:
        host = load_package().load_host()
        cfg = host_cfg(tiny_config(*MODES[mode], n_heads=4, n_kv_heads=2, n_layers=2, max_ctx=max_ctx))
        b = host.batch(cfg, n_seq)
        for i in range(len(cfg.weight_shapes())):
            b.set_weight(i, host.synth_weight(cfg, 4711, i))
        _models[key] = (host, cfg, b)
    return _models[key]


class Lists:
    """lists(prefix) of one prompt without any beam code: the prompt prefilled on sequence `seq` by the call the search uses, the
    prefix teacher-forced with decode_begin / decode_step_ragged, gten_hip_row_top_logprobs on that step's logits.  Memoised; `rows`
    keeps the raw logits rows."""

    def __init__(self, hip, b, cfg, prompt, n_top, seq=0):
        self.hip, self.b, self.cfg, self.prompt, self.n_top, self.seq = hip, b, cfg, list(prompt), n_top, seq
        self.memo, self.rows = {}, {}

    def __call__(self, prefix):
        if prefix not in self.memo:
            b, P, V = self.b, len(self.prompt), self.cfg.n_vocab
            b.prefill(self.seq, self.prompt, want=False)
            for q in range(b.n_seq):
                b.decode_begin(q, self.prompt + list(prefix) if q == self.seq else [0])
            for n in range(P, P + len(prefix) + 1):
                b.decode_step_ragged([n if q == self.seq else 1 for q in range(b.n_seq)])
            row = b.logits(self.seq)
            _, ti, tl = self.hip.row_top_logprobs(dev(self.hip, row), 1, V, V, -1, self.n_top)
            self.memo[prefix], self.rows[prefix] = (ti[0], tl[0]), row
        return self.memo[prefix]


def same_hyps(got, want, scores=True):
    assert len(got) == len(want), (got, want)
    for (gi, gf, gc, ge), (wi, wf, wc, we) in zip(got, want):
        assert gi.tolist() == wi and ge == we, (got, want)
        if scores:
            assert bits(gf) == bits(wf) and bits(gc) == bits(wc), (got, want)


def prompts_for(host, cfg, G, seed, lo=17, hi=30):
    r = np.random.default_rng(seed)
    return [list(host.synthetic_tokens(int(r.integers(lo, hi + 1)), seed=seed * 10 + g, n_vocab=cfg.n_vocab)) for g in range(G)]


def gather_mattered(parent_rows, B):
    """a round t >= 2 other than the search's last whose parent row is not the identity and names a beam twice: the gather copied
    rows between sets that differ (round 1 does not count: one source, and its rows are equal in every set) and a later step read them"""
    return any(p[:B].tolist() != list(range(B)) and len(set(p[:B].tolist())) < B for p in parent_rows[1:-1])


@pytest.mark.parametrize("mode", ["q4", "q8", "f16"])
@pytest.mark.parametrize("shape", [(4, 1, 4), (8, 2, 3)])
def test_whole_search_narrow_equals_the_reference_bit_for_bit(hip, mode, shape):
    n_seq, G, B = shape
    host, cfg, b = batch_of(mode, n_seq)
    w = ref.weights(MAX_NEW, 1.0)
    prompts = prompts_for(host, cfg, G, 31)
    lists = [Lists(hip, b, cfg, p, 2 * B) for p in prompts]
    first = [ref.search(lists[g], B, MAX_NEW, -1, w) for g in range(G)]
    got = b.beam_search(prompts, B, MAX_NEW)
    for g in range(G):
        assert all(h[3] == "length" and len(h[0]) == MAX_NEW for h in first[g][3])
        same_hyps(got[g], first[g][3])
    # once more with eos = the best beam's id at round 3 of that run (of the first prompt): hypotheses finish
    eos = int(first[0][2][2][0])
    second = [ref.search(lists[g], B, MAX_NEW, eos, w) for g in range(G)]
    got, rounds = b.beam_search_rc(prompts, B, MAX_NEW, eos)[1:]
    for g in range(G):
        same_hyps(got[g], second[g][3])
    assert rounds == max(int(s[0]["t"]) for s in second)
    print(f"{mode} {shape}: parent rows from round 2 on: {[[p[:B].tolist() for p in s[1][1:]] for s in first + second]}")
    assert any(gather_mattered(s[1], B) for s in first), "no round from 2 on duplicated a parent: choose another seed"
    assert any(gather_mattered(s[1], B) for s in second), "no round from 2 on duplicated a parent with eos set: choose another seed"
    assert any(h[3] == "eos" for s in second for h in s[3]), "no hypothesis ended by eos: choose another seed"
    # a length penalty other than 1 and a prompt below 16 ids
    w2 = ref.weights(4, 0.6)
    short = [p[:9] for p in prompts]
    l2 = [Lists(hip, b, cfg, p, 2 * B) for p in short]
    got = b.beam_search(short, B, 4, eos, 0.6)
    for g in range(G):
        same_hyps(got[g], ref.search(l2[g], B, 4, eos, w2)[3])


@pytest.mark.parametrize("mode", ["q4", "f16"])
def test_one_beam_is_greedy_generation(hip, mode):
    host, cfg, b = batch_of(mode, 4)
    prompts = prompts_for(host, cfg, 4, 57)
    P = [len(p) for p in prompts]
    greedy = b.generate(prompts, max(P) + MAX_NEW)
    got = b.beam_search(prompts, 1, MAX_NEW)
    for q in range(4):
        assert len(got[q]) == 1 and got[q][0][0].tolist() == greedy[q][P[q]: P[q] + MAX_NEW].tolist() and got[q][0][3] == "length"
    # an eos that comes up: sequence 0's third new id
    eos = int(greedy[0][P[0] + 2])
    greedy = b.generate(prompts, max(P) + MAX_NEW, eos)
    got = b.beam_search(prompts, 1, MAX_NEW, eos)
    for q in range(4):
        want = greedy[q][P[q]: P[q] + MAX_NEW].tolist()
        assert got[q][0][0].tolist() == want, (q, got[q], want)
        assert got[q][0][3] == ("eos" if len(want) < MAX_NEW else "length")
    assert got[0][0][3] == "eos" and len(got[0][0][0]) <= 2          # (at its first occurrence: the id may come up before position 2)


@pytest.mark.parametrize("mode", ["q8", "f16"])
def test_whole_search_wide_with_shadows(hip, mode):
    """16 sequences (head-major shadows on), 4 groups x 4 beams, against the reference replayed on the same batch: a sequence's bits
    do not depend on its slot, so ids and scores are held bit for bit"""
    host, cfg, b = batch_of(mode, 16)
    assert b.kv_info()[0] == 1                                           # the shadows are on
    G, B = 4, 4
    w = ref.weights(MAX_NEW, 1.0)
    prompts = prompts_for(host, cfg, G, 77, 17, 40)
    lists = [Lists(hip, b, cfg, p, 2 * B, seq=(5 * g + 3) % 16) for g, p in enumerate(prompts)]
    first = [ref.search(lists[g], B, MAX_NEW, -1, w) for g in range(G)]
    eos = int(first[1][2][2][0])
    second = [ref.search(lists[g], B, MAX_NEW, eos, w) for g in range(G)]
    imports = b.kv_info()[1]
    got = b.beam_search(prompts, B, MAX_NEW)
    print(f"{mode}: shadow imports during one search of {G} x {B} beams, {MAX_NEW} rounds: {b.kv_info()[1] - imports}")
    for g in range(G):
        same_hyps(got[g], first[g][3])
    got = b.beam_search(prompts, B, MAX_NEW, eos)
    for g in range(G):
        same_hyps(got[g], second[g][3])
    assert any(h[3] == "eos" for s in second for h in s[3])
    print(f"{mode}: parent rows from round 2 on: {[[p[:B].tolist() for p in s[1][1:]] for s in first + second]}")
    assert sum(gather_mattered(s[1], B) for s in first) >= 2, "the gather moved rows in fewer than two groups: choose another seed"


def test_afterwards_nothing_has_changed(hip):
    host, cfg, b = batch_of("q4", 8)
    prompts = prompts_for(host, cfg, 8, 91)
    queue = prompts_for(host, cfg, 13, 92)
    total = 30 + 8
    b.set_logprobs(1, 5)
    b.set_logprobs(6, 0)
    gen = b.generate(prompts, total)
    srv = b.serve(queue, total, max_new=7)[0]
    dec = b.fsm_decoder()
    info = hip.decoder_beam_info(dec)
    b.beam_search(prompts[:2], 3, MAX_NEW, int(gen[0][len(prompts[0]) + 2]))
    assert hip.decoder_beam_info(dec)[2] > info[2]
    tops = np.zeros(8, np.int32)
    hip._check(hip._logprobs_info(dec, None, tops.ctypes.data, None, None, None))
    assert tops.tolist() == [-1, 5, -1, -1, -1, -1, 0, -1]
    assert [g.tolist() for g in b.generate(prompts, total)] == [g.tolist() for g in gen]
    assert [s.tolist() for s in b.serve(queue, total, max_new=7)[0]] == [s.tolist() for s in srv]
    b.set_logprobs(1, -1)
    b.set_logprobs(6, -1)
    b.beam_search(prompts[:1], 8, 3)
    assert [g.tolist() for g in b.generate(prompts, total)] == [g.tolist() for g in gen]
    assert hip._dec_beam_round(dec) != 0 and "no search begun" in hip.last_error()


def test_refusals(hip):
    pkg = load_package()
    host, cfg, b = batch_of("q4", 8)
    V = cfg.n_vocab
    prompts = prompts_for(host, cfg, 2, 93)
    dec = b.fsm_decoder()
    w = ref.weights(MAX_NEW, 1.0)
    rc = lambda groups, w=w: hip.decoder_beam_begin(dec, groups, w)           # noqa: E731
    P = 20
    refused = [([(0, 0, P, 6, -1)], "beams"), ([(0, 9, P, 6, -1)], "beams"), ([(0, 3, P, 6, -1), (2, 3, P, 6, -1)], "two groups"),
               ([(6, 3, P, 6, -1)], "sequences"), ([(0, 2, 60, 6, -1)], "max_ctx"), ([(0, 2, 0, 6, -1)], "max_ctx"), ([(0, 2, P, 0, -1)], "max_ctx"),
               ([(0, 2, P, 6, V)], "eos")]
    for groups, word in refused:
        assert rc(groups) != 0 and word in hip.last_error(), (groups, hip.last_error())
    assert rc([(0, 2, P, 6, -1)], w[:6]) != 0 and "length weights" in hip.last_error()
    # the host call: the same refusals, nothing computed
    assert b.beam_search_rc(prompts, 9, MAX_NEW)[0] != 0 and "beams" in hip.last_error()
    assert b.beam_search_rc(prompts, 5, MAX_NEW)[0] != 0 and "sequences" in hip.last_error()      # 2 x 5 beams on 8 sequences
    assert b.beam_search_rc([prompts[0] + prompts[1] + prompts[0]], 2, MAX_NEW)[0] != 0 and "max_ctx" in hip.last_error()
    assert b.beam_search_rc(prompts, 2, 0)[0] == -1
    # a sequence that samples, is bound to a table or an automaton, or is penalised
    b.set_sampling(1, 40, 0.8, 1, 1)
    assert rc([(0, 2, P, 6, -1)]) != 0 and "sampling" in hip.last_error()
    assert rc([(2, 2, P, 6, -1)]) == 0 and hip.decoder_beam_end(dec) == 0      # (another sequence's request does not matter)
    b.set_sampling(1, 0)
    b.set_bias_table(1, [(3, -np.inf)])
    b.set_seq_bias(1, 1)
    assert rc([(0, 2, P, 6, -1)]) != 0 and "bias table" in hip.last_error()
    b.set_seq_bias(1, -1)
    b.set_penalty(0, 1.3)
    assert rc([(0, 2, P, 6, -1)]) != 0 and "penalised" in hip.last_error()
    b.set_penalty(0, 1.0)
    fsm = pkg.hostabi.Fsm(host, V)
    start = fsm.add_stop([[5, 6]])
    b.set_fsm(fsm)
    b.set_seq_fsm(1, start, 1)
    assert rc([(0, 2, P, 6, -1)]) != 0 and "automaton" in hip.last_error()
    b.set_seq_fsm(1, -1)
    # 2 * n_beams > n_vocab: a vocabulary of 8 ids
    small = host_cfg(tiny_config(Q4, Q8, n_heads=4, n_kv_heads=2, n_layers=2, max_ctx=64, n_vocab=8))
    sb = host.batch(small, 8)
    for i in range(len(small.weight_shapes())):
        sb.set_weight(i, host.synth_weight(small, 4711, i))
    assert hip.decoder_beam_begin(sb.fsm_decoder(), [(0, 5, P, 6, -1)], w) != 0 and "vocabulary" in hip.last_error()
    assert hip.decoder_beam_begin(sb.fsm_decoder(), [(0, 4, P, 6, -1)], w) == 0
    assert hip.decoder_beam_begin(sb.fsm_decoder(), [(4, 4, P, 6, -1)], w) != 0 and "already begun" in hip.last_error()
    assert hip.decoder_beam_end(sb.fsm_decoder()) == 0
    sb.close()
    # everything refused left the batch as it was
    assert len(b.beam_search(prompts, 2, MAX_NEW)[0]) == 2
