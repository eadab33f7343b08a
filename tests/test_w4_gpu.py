"""-m gpu: GPTQ / AWQ 4-bit tensors unpacked and transposed on the device while they are quantised (include/gten_hip_w4.h, DESIGN.md
§3.30), byte for byte against tests/w4_ref.py's NumPy dequantisation run through the converter: every destination, layout and
shape of the issue, the refusals, and a small model loaded from a safetensors checkpoint against the operator-level expectation."""
import functools
import importlib
import json

import numpy as np
import pytest

import w4_ref
from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

load_package()
convert = importlib.import_module("tinyllama_cpp_amd.convert")
CODES = {"f16": 1, "q8": 3, "q4": 4}
# (layout, zero_offset, act-order): GPTQ v1 | GPTQ v2 with a random g_idx (blocks straddle groups) | AWQ
LAYOUTS = [("gptq", 1, False), ("gptq", 0, True), ("awq", 0, False)]
# (N, K, group).  Tiles are 64 x 256 (GPTQ) and 256 x 256 (AWQ): one block, everything else surplus | N = 64 + 8 and K < 256: a partial
# tile in both directions for both layouts, AWQ rows of 9 words (4-byte requests) | N = 4 x 64 + 8 = 256 + 8, K = 256 + 128, 3 groups |
# one full GPTQ tile, one group, AWQ rows of 8 words (16-byte requests)
SHAPES = [(8, 32, 32), (72, 160, 32), (264, 384, 128), (64, 256, -1)]


@functools.lru_cache(maxsize=None)
def case(layout, zero_offset, act, n, k, group):
    """(the four source tensors, D), computed once per layout and shape"""
    src = w4_ref.random_source(layout, n, k, group, np.random.default_rng(n * 1009 + k + act), act)
    d = w4_ref.dequant(layout, *src, zero_offset, group)
    d.setflags(write=False)
    return src, d


@pytest.mark.parametrize("n, k, group", SHAPES)
@pytest.mark.parametrize("layout, zero_offset, act", LAYOUTS)
@pytest.mark.parametrize("dst", ["q8", "q4", "f16"])
def test_quantize_weight_w4_is_pack_of_the_converter_on_the_dequantised_matrix(hip, dst, layout, zero_offset, act, n, k, group):
    src, d = case(layout, zero_offset, act, n, k, group)
    assert [hip.w4_src_bytes(layout, which, n, k, group) for which in range(4)] == [a.nbytes for a in src[:3]] + [4 * k if layout == "gptq" else 0]
    got_buf = hip.quantize_weight_w4(*src, layout, zero_offset, n, k, group, CODES[dst])
    got = got_buf.download()
    got_buf.free()
    if dst == "f16":
        want = convert.to_f16(d).reshape(-1)
    else:
        want_buf = hip.upload_weight(convert.quantize(d, dst, "f16"), CODES[dst], n, k)
        want = want_buf.download()
        want_buf.free()
    assert got.size == n * hip.row_bytes(CODES[dst], k)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("layout, zero_offset, act", LAYOUTS)
def test_an_infinite_scale_is_refused_and_the_next_call_succeeds(hip, layout, zero_offset, act):
    Err = load_package().hipabi.GtenHipError
    (qweight, qzeros, scales, g_idx), _ = case(layout, zero_offset, act, 264, 384, 128)
    bad = scales.copy()
    bad[2, 201] = np.inf                                        # the last group, a row of the fourth GPTQ tile: far from element 0
    with pytest.raises(Err, match="quantize_weight_w4.*NaN or an infinity"):
        hip.quantize_weight_w4(qweight, qzeros, bad, g_idx, layout, zero_offset, 264, 384, 128, CODES["q4"])
    hip.quantize_weight_w4(qweight, qzeros, scales, g_idx, layout, zero_offset, 264, 384, 128, CODES["q4"]).free()      # the flag is down again


def test_a_g_idx_entry_equal_to_the_number_of_groups_is_refused(hip):
    Err = load_package().hipabi.GtenHipError
    (qweight, qzeros, scales, g_idx), _ = case("gptq", 0, True, 264, 384, 128)
    bad = g_idx.copy()
    bad[300] = 3
    with pytest.raises(Err, match=r"quantize_weight_w4: g_idx holds an entry outside \[0, 3\)"):
        hip.quantize_weight_w4(qweight, qzeros, scales, bad, "gptq", 0, 264, 384, 128, CODES["q8"])
    hip.quantize_weight_w4(qweight, qzeros, scales, g_idx, "gptq", 0, 264, 384, 128, CODES["q8"]).free()
    assert hip.w4_src_bytes("gptq", 0, 264, 384, 96) == 264 * 384 // 2 and hip.w4_src_bytes("gptq", 0, 264, 384, 100) == 0
    assert hip.w4_src_bytes("awq", 0, 260, 384, 128) == 0 and hip.w4_src_bytes("awq", 0, 264, 400, -1) == 0 and hip.w4_src_bytes("awq", 4, 264, 384, -1) == 0


@pytest.mark.parametrize("layout, zero_offset, act", LAYOUTS)
def test_load_quantized_leaves_the_operator_level_weights(hip, tmp_path, layout, zero_offset, act):
    """a 2-layer model from a safetensors checkpoint with random 4-bit linears (group 128) and f16 embed_tokens / lm_head / norms:
    every weight_read and the logits of a prompt equal the model filled from the reference's dequantisation"""
    from safetensors.numpy import save_file
    host = load_package().load_host()
    cfg = host.default_config(CODES["q4"], 3)
    cfg.n_vocab, cfg.max_ctx, cfg.n_embd, cfg.n_ffn, cfg.n_layers, cfg.n_heads, cfg.n_kv_heads = 515, 64, 256, 512, 2, 4, 2
    rng = np.random.default_rng(31)
    names = [n for n, _ in convert.tensor_names(cfg.n_layers)]
    tensors, want = {}, {}
    for name, (rows, cols, dt) in zip(names, cfg.weight_shapes()):
        if dt == 1 or "layers" not in name:
            w = (rng.standard_normal((1, cols) if dt == 1 else (rows, cols)) * (1 if dt == 1 else 0.02)).astype(np.float16)
            tensors[name] = w.reshape(-1) if dt == 1 else w
            want[name] = convert.to_f16(w.astype(np.float32)) if dt == 1 else convert.quantize(w.astype(np.float32), "q4", "f16")
            continue
        src = w4_ref.random_source(layout, rows, cols, 128, rng, act, scale_max=0.005)        # (weights of a few hundredths: the logits stay finite)
        tensors.update({f"{name[:-7]}.{part}": a for part, a in zip(("qweight", "qzeros", "scales", "g_idx"), src) if a is not None})
        want[name] = convert.quantize(w4_ref.dequant(layout, *src, zero_offset, 128), "q4", "f16")
    save_file(tensors, str(tmp_path / "model.safetensors"))
    qc = {"quant_method": layout, "bits": 4, "group_size": 128, "desc_act": act, "sym": False, "version": "gemm", "checkpoint_format": "gptq" if zero_offset else "gptq_v2"}
    (tmp_path / "config.json").write_text(json.dumps({"quantization_config": qc}))
    a, b = host.model(cfg), host.model(cfg)
    for i, name in enumerate(names):
        a.set_weight(i, want[name])
    b.load_quantized(str(tmp_path))
    same = [np.array_equal(a.weight_read(i), b.weight_read(i)) for i in range(a.n_weights())]
    prompt = rng.integers(0, cfg.n_vocab, 12).astype(np.int32)
    la, lb = a.logits(prompt, 0), b.logits(prompt, 0)
    a.close()
    b.close()
    assert all(same), [names[i] for i, ok in enumerate(same) if not ok]
    assert np.isfinite(la).all() and la.std() > 0 and la.tobytes() == lb.tobytes()
