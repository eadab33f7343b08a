"""-m gpu: the o launch as four K-quarter planes (k_dec_o_planes, csrc/gten_decode_oplanes.h; gten_hip_set_decode_o_planes,
include/gten_hip_oplanes.h) must not change a bit.  Two single-sequence decoders on the same weights -- the control (one plane: every
workgroup joins and stages the whole vector) and the planes -- give the same ids at every n = 1 .. 2048 and the same logits, bit for
bit, at n in {1, 2, 255, 256, 257, 512, 513, 1793, 2047, 2048}: one, two, three and eight chunks of the attention and the boundaries
where a chunk's partials are still stale.  Graph replay and eager launches alternate; decode_steps (four steps per graph) across
254 -> 262 and 2040 -> 2048 gives the ids of the single steps.  All of it with no weights resident and with every W.x launch resident
(both cache policies of the weight requests), in q4 and q8.

The smallest shape the planes accept: n_embd 2048, 32 heads of 64, 4 kv heads, 2 layers (the plane buffer is reused from layer to
layer), n_ffn 512, the small vocabulary, max_ctx 2048.  An f16 model, an n_embd-512 model, a decoder of 8 sequences and an exact-form
decoder report 0 whatever the setting, and decode the same ids under both.  Everything is equality."""
import numpy as np
import pytest

from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from helpers import MODES, tiny_config
from test_model_gpu import host_cfg

pytestmark = pytest.mark.gpu

WATCH = (1, 2, 255, 256, 257, 512, 513, 1793, 2047, 2048)
N = 2048
E, H, KV, L, F = 2048, 32, 4, 2, 512
STEPS_AT = ((254, 9), (2040, 9))                # decode_steps(first, count): 254 -> 262, 2040 -> 2048
QUANT = [m for m in MODES() if m[0] in ("q4", "q8")]
BUDGETS = {"none": 0, "all": 1024}              # MiB: nothing resident | far more than these weights

_setups, _runs = {}, {}


def _setup(wd, ad, n_embd=E, n_heads=H, n_kv=KV, max_ctx=N):
    key = (wd, ad, n_embd, n_heads, n_kv, max_ctx)
    if key not in _setups:
        host = load_package().load_host()
        cfg = host_cfg(tiny_config(wd, ad, n_embd=n_embd, n_ffn=F, n_heads=n_heads, n_kv_heads=n_kv, n_layers=L, max_ctx=max_ctx))
        toks = host.synthetic_tokens(max_ctx, seed=2048, n_vocab=cfg.n_vocab)
        weights = [host.synth_weight(cfg, 717, i) for i in range(len(cfg.weight_shapes()))]
        _setups[key] = (host, cfg, toks, weights)
    return _setups[key]


class _settings:
    """the o-planes switch and the resident budget while a decoder is created (both are read then), put back afterwards"""

    def __init__(self, hip, planes, mb=None, exact=False):
        self.hip, self.planes, self.mb, self.exact = hip, planes, mb, exact

    def __enter__(self):
        self.before = self.hip.weight_resident_bytes()
        self.planes_before = self.hip.decode_o_planes()
        self.hip.set_decode_o_planes(self.planes)
        if self.mb is not None:
            self.hip.set_weight_resident_mb(self.mb)
        if self.exact:
            self.hip.set_decode_exact(True)

    def __exit__(self, *exc):
        if self.exact:
            self.hip.set_decode_exact(False)
        self.hip.set_weight_resident_bytes(self.before)
        self.hip.set_decode_o_planes(self.planes_before)
        return False


def _model(hip, setup, planes, mb=None, exact=False):
    """(model, what its decoder reports: o planes, resident launches)"""
    host, cfg, _, weights = setup
    with _settings(hip, planes, mb, exact):
        gm = host.model(cfg)
        try:
            for i, w in enumerate(weights):
                gm.set_weight(i, w)
            report = (gm.o_planes(), gm.resident()[0])          # (creates the decoder)
        except Exception:
            gm.close()
            raise
    return gm, report


def _single_steps(hip, name, wd, ad, planes, budget):
    """(ids of steps 1 .. N, logits at WATCH, the decoder's report) of one decoder, one step per call; computed once"""
    key = (name, planes, budget)
    if key not in _runs:
        setup = _setup(wd, ad)
        toks = setup[2]
        gm, report = _model(hip, setup, planes, BUDGETS[budget])
        try:
            gm.decode_begin(toks)
            ids, logits = [], {}
            for n in range(1, N + 1):
                gm.decode_step(n, n % 2 == 0)       # alternate graph replay and eager launches
                ids.append(gm.decode_result(n))
                if n in WATCH:
                    logits[n] = gm.logits(toks[:n], n - 1).copy()
        finally:
            gm.close()
        _runs[key] = (ids, logits, report)
    return _runs[key]


@pytest.mark.parametrize("budget", sorted(BUDGETS))
@pytest.mark.parametrize("name,wd,ad", QUANT)
def test_the_planes_do_not_change_a_bit(hip, name, wd, ad, budget):
    cfg = _setup(wd, ad)[1]
    ids0, lg0, rep0 = _single_steps(hip, name, wd, ad, 0, budget)
    ids1, lg1, rep1 = _single_steps(hip, name, wd, ad, 1, budget)
    resident = 4 * cfg.n_layers + 1 if budget == "all" else 0
    assert rep0 == (0, resident) and rep1 == (1, resident), (name, budget, rep0, rep1)
    assert len(ids0) == N and ids0 == ids1, (name, budget, next(i + 1 for i in range(N) if ids0[i] != ids1[i]))
    assert len(set(ids0)) > 8                        # the ids are a function of the context, not a constant
    for n in WATCH:
        assert np.isfinite(lg0[n]).all(), (name, budget, n)
        assert np.array_equal(lg0[n].view(np.uint32), lg1[n].view(np.uint32)), (name, budget, n)


@pytest.mark.parametrize("budget", sorted(BUDGETS))
@pytest.mark.parametrize("name,wd,ad", QUANT)
def test_four_step_graphs_across_the_chunk_boundaries(hip, name, wd, ad, budget):
    want = _single_steps(hip, name, wd, ad, 0, budget)[0]
    setup = _setup(wd, ad)
    toks = setup[2]
    gm, report = _model(hip, setup, 1, BUDGETS[budget])
    got = {}
    try:
        assert report[0] == 1
        gm.decode_begin(toks)
        n = 1
        for first, count in STEPS_AT:
            while n < first:
                gm.decode_step(n, True)
                n += 1
            gm.decode_steps(first, count, True)      # four steps per graph replay
            for m in range(first, first + count):
                got[m] = gm.decode_result(m)
            n = first + count
    finally:
        gm.close()
    assert len(got) == sum(c for _, c in STEPS_AT) and max(got) == N
    for m, i in got.items():
        assert i == want[m - 1], (name, budget, m)


def _few_ids(gm, toks, steps=3):
    gm.decode_begin(toks)
    out = []
    for n in range(1, steps + 1):
        gm.decode_step(n, n % 2 == 0)
        out.append(gm.decode_result(n))
    return out


@pytest.mark.parametrize("what", ["f16", "n_embd_512", "exact"])
def test_other_single_sequence_decoders_keep_one_plane(hip, what):
    by_name = {m[0]: m for m in MODES()}
    if what == "f16":
        setup, exact = _setup(by_name["f16"][1], by_name["f16"][2], max_ctx=64), False
    elif what == "n_embd_512":
        setup, exact = _setup(by_name["q4"][1], by_name["q4"][2], n_embd=512, n_heads=8, n_kv=2, max_ctx=64), False
    else:
        setup, exact = _setup(by_name["q4"][1], by_name["q4"][2], max_ctx=64), True
    ids = []
    for planes in (0, 1):
        gm, report = _model(hip, setup, planes, exact=exact)
        try:
            assert report[0] == 0, (what, planes)
            ids.append(_few_ids(gm, setup[2]))
        finally:
            gm.close()
    assert ids[0] == ids[1]


def test_a_decoder_of_eight_sequences_keeps_one_plane(hip):
    q4 = {m[0]: m for m in MODES()}["q4"]
    host, cfg, toks, weights = _setup(q4[1], q4[2], max_ctx=64)
    ids = []
    for planes in (0, 1):
        with _settings(hip, planes):
            b = host.batch(cfg, 8)
            try:
                for i, w in enumerate(weights):
                    b.set_weight(i, w)
                assert b.o_planes() == 0, planes
                for q in range(8):
                    b.decode_begin(q, np.roll(toks, q))
                got = []
                for n in range(1, 4):
                    b.decode_step(n, n % 2 == 0)
                    got.append([b.decode_result(q, n) for q in range(8)])
                ids.append(got)
            finally:
                b.close()
    assert ids[0] == ids[1]


def test_another_value_is_refused(hip):
    before = hip.decode_o_planes()
    assert before in (0, 1)
    for v in (2, -1):
        with pytest.raises(Exception):
            hip.set_decode_o_planes(v)
    assert hip.decode_o_planes() == before           # a refused value leaves the setting alone
    setup = _setup(*{m[0]: m for m in MODES()}["q4"][1:], max_ctx=64)
    gm, report = _model(hip, setup, 1)              # one chunk of context: the planes take it too
    gm.close()
    assert report[0] == 1 and hip.decode_o_planes() == before
