"""-m gpu: the single-sequence attention kernel k_dec_attn_one64v against k_dec_attn_one64, the A/B control that
gten_hip_set_decode_attn_classic(1) selects (include/gten_hip.h).

Both kernels promise the same partials and statistics at every context length, so the decoder's ids and logits must be
bit-identical: n from 1 to 2048 (ragged last chunks, the partial Q8 tail block of the probabilities, the chunk boundaries),
grouped-query shapes 4 / 2, 8 / 2 and 32 / 4 with d_head 64, every dtype, graph replay and eager launches alternating."""
import numpy as np
import pytest

from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from helpers import MODES, tiny_config
from test_model_gpu import host_cfg

pytestmark = pytest.mark.gpu

WATCH = (1, 2, 31, 32, 33, 255, 256, 257, 300, 511, 512, 2047, 2048)
N = max(WATCH)
# (n_embd, n_heads, n_kv_heads, n_layers): d_head 64 everywhere
SHAPES = {"gqa4_2": (256, 4, 2, 2), "gqa8_2": (512, 8, 2, 2), "gqa32_4": (2048, 32, 4, 1)}


def _run(hip, host, cfg, weights, toks, classic):
    hip.set_decode_attn_classic(classic)            # (read when the decoder is created)
    try:
        gm = host.model(cfg)
        try:
            for i, w in enumerate(weights):
                gm.set_weight(i, w)
            gm.decode_begin(toks)
            ids, logits = [], {}
            for n in range(1, N + 1):
                gm.decode_step(n, n % 2 == 0)       # alternate graph replay and eager launches
                ids.append(gm.decode_result(n))
                if n in WATCH:
                    logits[n] = gm.logits(toks[:n], n - 1).copy()
        finally:
            gm.close()
    finally:
        hip.set_decode_attn_classic(False)
    return ids, logits


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("name,wd,ad", MODES())
def test_new_attention_kernel_is_bit_identical_to_the_classic_one(hip, shape, name, wd, ad):
    E, H, KV, L = SHAPES[shape]
    host = load_package().load_host()
    cfg = host_cfg(tiny_config(wd, ad, n_embd=E, n_ffn=512, n_heads=H, n_kv_heads=KV, n_layers=L, max_ctx=N))
    toks = host.synthetic_tokens(N, seed=4242, n_vocab=cfg.n_vocab)
    weights = [host.synth_weight(cfg, 313, i) for i in range(len(cfg.weight_shapes()))]
    ids_new, lg_new = _run(hip, host, cfg, weights, toks, False)
    ids_old, lg_old = _run(hip, host, cfg, weights, toks, True)
    assert ids_new == ids_old, (name, shape)
    for n in WATCH:
        assert np.isfinite(lg_new[n]).all(), (name, shape, n)
        assert np.array_equal(lg_new[n].view(np.uint32), lg_old[n].view(np.uint32)), (name, shape, n)
