"""-m gpu: the three single-sequence attention kernels that gten_hip_set_decode_attn_classic selects (include/gten_hip_ab.h) --
0: k_dec_attn_one64w (the default: the softmax chain on waves 0-3, V widened and the new k / v rows appended by helper waves
4-7), 1: k_dec_attn_one64, 2: k_dec_attn_one64v -- write the same partials, statistics and cache rows, so the decoder's ids
and logits are bit-identical whichever runs.

Small shapes, n from 1 to 520: the helper-wave row boundaries (63 / 64 / 65, 255 / 256 / 257, 319 / 320), the chunk
boundaries, the new position as the first or the last row of a chunk (the V-row patch and the writer's append), a ragged last
chunk with a partial Q8 tail block of the probabilities; graph replay and eager launches alternating.  One more case takes the
default kernel through decode_steps (four steps per graph) across both chunk boundaries.  Everything is equality."""
import numpy as np
import pytest

from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from helpers import MODES, tiny_config
from test_model_gpu import host_cfg

pytestmark = pytest.mark.gpu

WATCH = (1, 2, 63, 64, 65, 255, 256, 257, 258, 319, 320, 511, 512, 513, 520)
N = max(WATCH)
# (n_embd, n_heads, n_kv_heads, n_layers): d_head 64
SHAPES = {"gqa4_2": (256, 4, 2, 2), "gqa8_2": (512, 8, 2, 2)}
STEPS_AT = ((254, 9), (510, 9))                 # decode_steps(first, count): 254 -> 262 and 510 -> 518

_setups, _runs = {}, {}


def _setup(shape, wd, ad):
    key = (shape, wd, ad)
    if key not in _setups:
        E, H, KV, L = SHAPES[shape]
        host = load_package().load_host()
        cfg = host_cfg(tiny_config(wd, ad, n_embd=E, n_ffn=512, n_heads=H, n_kv_heads=KV, n_layers=L, max_ctx=N))
        toks = host.synthetic_tokens(N, seed=4242, n_vocab=cfg.n_vocab)
        weights = [host.synth_weight(cfg, 313, i) for i in range(len(cfg.weight_shapes()))]
        _setups[key] = (host, cfg, toks, weights)
    return _setups[key]


def _model(hip, setup, mode):
    host, cfg, _, weights = setup
    hip.set_decode_attn_classic(mode)               # (read when the decoder is created)
    gm = host.model(cfg)
    for i, w in enumerate(weights):
        gm.set_weight(i, w)
    return gm


def _single_steps(hip, shape, wd, ad, mode):
    """(ids of steps 1 .. N, logits at WATCH) of one decoder in `mode`, one step per call; computed once per mode"""
    key = (shape, wd, ad, mode)
    if key not in _runs:
        setup = _setup(shape, wd, ad)
        toks = setup[2]
        try:
            gm = _model(hip, setup, mode)
            try:
                gm.decode_begin(toks)
                ids, logits = [], {}
                for n in range(1, N + 1):
                    gm.decode_step(n, n % 2 == 0)   # alternate graph replay and eager launches
                    ids.append(gm.decode_result(n))
                    if n in WATCH:
                        logits[n] = gm.logits(toks[:n], n - 1).copy()
            finally:
                gm.close()
        finally:
            hip.set_decode_attn_classic(0)
        _runs[key] = (ids, logits)
    return _runs[key]


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("name,wd,ad", MODES())
def test_three_attention_kernels_write_the_same_bytes(hip, shape, name, wd, ad):
    ids0, lg0 = _single_steps(hip, shape, wd, ad, 0)
    for mode in (1, 2):
        ids, lg = _single_steps(hip, shape, wd, ad, mode)
        assert ids0 == ids, (name, shape, mode)
        for n in WATCH:
            assert np.isfinite(lg0[n]).all(), (name, shape, n)
            assert np.array_equal(lg0[n].view(np.uint32), lg[n].view(np.uint32)), (name, shape, mode, n)


@pytest.mark.parametrize("name,wd,ad", MODES())
def test_default_kernel_in_four_step_graphs_across_the_chunk_boundaries(hip, name, wd, ad):
    shape = "gqa4_2"
    want, _ = _single_steps(hip, shape, wd, ad, 2)
    setup = _setup(shape, wd, ad)
    toks = setup[2]
    got = {}
    try:
        gm = _model(hip, setup, 0)
        try:
            gm.decode_begin(toks)
            n = 1
            for first, count in STEPS_AT:
                while n < first:
                    gm.decode_step(n, True)
                    n += 1
                gm.decode_steps(first, count, True)  # four steps per graph replay
                for m in range(first, first + count):
                    got[m] = gm.decode_result(m)
                n = first + count
        finally:
            gm.close()
    finally:
        hip.set_decode_attn_classic(0)
    assert len(got) == sum(c for _, c in STEPS_AT)
    for m, i in got.items():
        assert i == want[m - 1], (name, m)


def test_mode_outside_0_1_2_is_refused(hip):
    with pytest.raises(Exception):
        hip.set_decode_attn_classic(3)
    hip.set_decode_attn_classic(0)
