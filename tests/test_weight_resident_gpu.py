"""-m gpu: the cache policy of a W.x launch's weight requests (gten_hip_set_weight_resident_mb, include/gten_hip_ab.h; the plan:
host/resident_plan.h) must not change a bit.  Three single-sequence decoders on the same weights -- budget 0 (every request
nontemporal), budget = everything (every W.x launch on the default policy), and a budget that splits a family (layer 0's down
resident, layer 1's not) -- give the same ids at every n = 1 .. 300 (across one chunk boundary) and the same logits, bit for bit, at
n in {1, 2, 255, 256, 257, 300}, graph replay and eager launches alternating; decode_steps (four steps per graph) across 254 -> 262
gives the ids of the single steps.  The small shapes of tests/test_decode_attn_helpers_gpu.py, in q4, q8 and f16.

Each decoder reports the launches and bytes that the CPU plan gives for the bytes it had left; a decoder of 8 sequences and an
exact-form decoder report none whatever the setting.  Everything is equality."""
import numpy as np
import pytest

from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from helpers import MODES, tiny_config
from test_model_gpu import host_cfg

pytestmark = pytest.mark.gpu

WATCH = (1, 2, 255, 256, 257, 300)
N = max(WATCH)
# (n_embd, n_heads, n_kv_heads, n_layers): d_head 64
SHAPES = {"gqa4_2": (256, 4, 2, 2), "gqa8_2": (512, 8, 2, 2)}
N_FFN = 512
STEPS_AT = (254, 9)                             # decode_steps(first, count): 254 -> 262
DOWN0, DOWN1 = 3, 7                             # the down launches of layers 0 and 1 in step order (q|k|v, o, gate|up, down per layer)

_setups, _runs = {}, {}


def _setup(shape, wd, ad):
    key = (shape, wd, ad)
    if key not in _setups:
        E, H, KV, L = SHAPES[shape]
        host = load_package().load_host()
        cfg = host_cfg(tiny_config(wd, ad, n_embd=E, n_ffn=N_FFN, n_heads=H, n_kv_heads=KV, n_layers=L, max_ctx=N))
        toks = host.synthetic_tokens(N, seed=4242, n_vocab=cfg.n_vocab)
        weights = [host.synth_weight(cfg, 313, i) for i in range(len(cfg.weight_shapes()))]
        _setups[key] = (host, cfg, toks, weights)
    return _setups[key]


def _plan(host, cfg, name, budget):
    E, H = cfg.n_embd, cfg.n_heads
    return host.resident_plan(cfg.n_layers, E, cfg.n_ffn, (E // H) * cfg.n_kv_heads, cfg.n_vocab, host.RESIDENT_BLOCK_BYTES[name], budget)


def _model(hip, setup, setting):
    """a model whose decoder is created under a setting of `setting` bytes (read when the decoder is created)"""
    host, cfg, _, weights = setup
    before = hip.weight_resident_bytes()
    hip.set_weight_resident_bytes(setting)
    try:
        gm = host.model(cfg)
        try:
            for i, w in enumerate(weights):
                gm.set_weight(i, w)
            info = gm.resident()                    # (creates the decoder)
        except Exception:
            gm.close()
            raise
    finally:
        hip.set_weight_resident_bytes(before)
    return gm, info


def _budgets(hip, shape, name, wd, ad):
    """{kind: the bytes left for the weights}: none, everything, and a budget that ends with layer 0's down"""
    setup = _setup(shape, wd, ad)
    host, cfg = setup[0], setup[1]
    _, each, _, _ = _plan(host, cfg, name, 0)
    order = sorted(range(len(each)), key=lambda i: (int(each[i]), i))
    assert order.index(DOWN0) < order.index(DOWN1)
    split = int(sum(int(each[i]) for i in order[: order.index(DOWN0) + 1]))
    res, _, _, _ = _plan(host, cfg, name, split)
    assert res[DOWN0] == 1 and res[DOWN1] == 0      # one of the two layers of down
    return {"none": 0, "all": int(each.sum()), "split": split}


def _single_steps(hip, shape, name, wd, ad, kind):
    """(ids of steps 1 .. N, logits at WATCH, what the decoder reports) of one decoder, one step per call; computed once per kind"""
    key = (shape, wd, ad, kind)
    if key not in _runs:
        setup = _setup(shape, wd, ad)
        toks = setup[2]
        left = _budgets(hip, shape, name, wd, ad)[kind]
        gm0, (_, _, _, overhead) = _model(hip, setup, 0)         # what a decoder of this shape takes off the setting first
        gm0.close()
        assert overhead > 0
        gm, info = _model(hip, setup, overhead + left if left else 0)
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
        _runs[key] = (ids, logits, info, left)
    return _runs[key]


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("name,wd,ad", MODES())
def test_the_load_policy_does_not_change_a_bit(hip, shape, name, wd, ad):
    host, cfg = _setup(shape, wd, ad)[:2]
    ids0, lg0, info0, _ = _single_steps(hip, shape, name, wd, ad, "none")
    assert info0[:3] == (0, 0, 0), info0
    for kind in ("all", "split"):
        ids, lg, (launches, nbytes, budget, overhead), left = _single_steps(hip, shape, name, wd, ad, kind)
        res, _, want_launches, want_bytes = _plan(host, cfg, name, left)
        assert budget == left and (launches, nbytes) == (want_launches, want_bytes), (name, shape, kind)
        assert launches == (4 * cfg.n_layers + 1 if kind == "all" else int(res.sum())) and 0 < launches
        assert ids0 == ids, (name, shape, kind)
        for n in WATCH:
            assert np.isfinite(lg0[n]).all(), (name, shape, n)
            assert np.array_equal(lg0[n].view(np.uint32), lg[n].view(np.uint32)), (name, shape, kind, n)


@pytest.mark.parametrize("kind", ["all", "split"])
@pytest.mark.parametrize("name,wd,ad", MODES())
def test_four_step_graphs_across_the_chunk_boundary(hip, name, wd, ad, kind):
    shape = "gqa4_2"
    want, _, _, _ = _single_steps(hip, shape, name, wd, ad, "none")
    setup = _setup(shape, wd, ad)
    toks = setup[2]
    left = _budgets(hip, shape, name, wd, ad)[kind]
    overhead = _single_steps(hip, shape, name, wd, ad, kind)[2][3]
    gm, info = _model(hip, setup, overhead + left)
    got = {}
    try:
        assert info[0] > 0
        gm.decode_begin(toks)
        first, count = STEPS_AT
        for n in range(1, first):
            gm.decode_step(n, True)
        gm.decode_steps(first, count, True)          # four steps per graph replay
        for m in range(first, first + count):
            got[m] = gm.decode_result(m)
    finally:
        gm.close()
    assert len(got) == STEPS_AT[1]
    for m, i in got.items():
        assert i == want[m - 1], (name, kind, m)


@pytest.mark.parametrize("name,wd,ad", MODES())
def test_wider_and_exact_decoders_keep_budget_zero(hip, name, wd, ad):
    setup = _setup("gqa4_2", wd, ad)
    host, cfg, _, weights = setup
    before = hip.weight_resident_bytes()
    hip.set_weight_resident_mb(64)                   # far more than these weights: a fast single-sequence decoder takes them all
    try:
        gm, info = _model(hip, setup, 64 << 20)
        gm.close()
        assert info[0] == 4 * cfg.n_layers + 1
        b = host.batch(cfg, 8)
        try:
            for i, w in enumerate(weights):
                b.set_weight(i, w)
            assert b.resident()[:3] == (0, 0, 0)
        finally:
            b.close()
        hip.set_decode_exact(True)
        try:
            gm = host.model(cfg)
            try:
                for i, w in enumerate(weights):
                    gm.set_weight(i, w)
                assert gm.resident()[:3] == (0, 0, 0)
            finally:
                gm.close()
        finally:
            hip.set_decode_exact(False)
    finally:
        hip.set_weight_resident_bytes(before)


def test_a_negative_budget_is_refused(hip):
    before = hip.weight_resident_bytes()
    with pytest.raises(Exception):
        hip.set_weight_resident_mb(-1)
    assert hip.weight_resident_bytes() == before
