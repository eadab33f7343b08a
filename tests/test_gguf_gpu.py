"""-m gpu: GGUF tensors decoded on the device while they are quantised (include/gten_hip_gguf.h), byte for byte
against tests/gguf_ref.py's NumPy dequantisation run through the converter: every format, destination and shape of the issue, the
non-finite refusal, the sizes; and a small model loaded from a GGUF file against the operator-level expectation."""
import functools
import importlib

import numpy as np
import pytest

import gguf_ref
from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu

load_package()
convert = importlib.import_module("tinyllama_cpp_amd.convert")
CODES = {"f16": 1, "q8": 3, "q4": 4}
SHAPES = [(3, 512, 0), (5, 768, 0), (32, 256, 2)]      # a full wave per row | surplus quads, rows at 2-byte offsets | the row map, D = 16


@functools.lru_cache(maxsize=None)
def case(code, rows, cols, n_head):
    """(block stream, its dequantisation in destination row order), computed once per format and shape"""
    stream = gguf_ref.random_stream(code, rows, cols, np.random.default_rng(code * 1009 + cols))
    x = gguf_ref.dequant(stream, code, rows, cols)[gguf_ref.row_map(rows, n_head)]
    x.setflags(write=False)
    return stream, x


@pytest.mark.parametrize("rows, cols, n_head", SHAPES)
@pytest.mark.parametrize("dst", ["q8", "q4", "f16"])
@pytest.mark.parametrize("code", sorted(gguf_ref.FORMATS))
def test_quantize_weight_gguf_is_pack_of_the_converter_on_the_dequantised_rows(hip, code, dst, rows, cols, n_head):
    stream, x = case(code, rows, cols, n_head)
    assert hip.gguf_src_bytes(code, rows, cols) == gguf_ref.src_bytes(code, rows, cols) == stream.size
    got_buf = hip.quantize_weight_gguf(stream, code, rows, cols, CODES[dst], n_head)
    got = got_buf.download()
    got_buf.free()
    if dst == "f16":
        want = convert.to_f16(x).reshape(-1)
    else:
        want_buf = hip.upload_weight(convert.quantize(x, dst, "f32"), CODES[dst], rows, cols)
        want = want_buf.download()
        want_buf.free()
    assert got.size == rows * hip.row_bytes(CODES[dst], cols)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("dst", ["q8", "q4", "f16"])
@pytest.mark.parametrize("code", sorted(gguf_ref.FORMATS))
def test_an_infinite_d_is_refused_and_other_types_and_shapes_have_no_size(hip, code, dst):
    Err = load_package().hipabi.GtenHipError
    stream = case(code, 5, 768, 0)[0].copy()
    unit = gguf_ref.FORMATS[code][1]
    at = 7 * unit + (208 if code == 14 else 0)                 # d of block 7: not the first of its wave or row
    stream[at:at + 2] = np.array([np.inf], np.float16).view(np.uint8)
    with pytest.raises(Err, match="quantize_weight_gguf.*NaN or an infinity"):
        hip.quantize_weight_gguf(stream, code, 5, 768, CODES[dst])
    good = hip.quantize_weight_gguf(case(code, 5, 768, 0)[0], code, 5, 768, CODES[dst])        # the flag is down again
    good.free()
    assert hip.gguf_src_bytes(code, 5, 768 + 32) == (0 if code >= 12 else gguf_ref.src_bytes(code, 5, 800))
    assert hip.gguf_src_bytes(code, 5, 48) == 0 and hip.gguf_src_bytes(11, 5, 768) == 0 and hip.gguf_src_bytes(code, 0, 768) == 0
    with pytest.raises(Err, match="ggml type 11 is not supported"):
        hip.quantize_weight_gguf(stream, 11, 5, 768, CODES[dst])


@pytest.mark.parametrize("with_output", [True, False])
def test_load_gguf_leaves_the_operator_level_weights(hip, tmp_path, with_output):
    """linears Q4_K, output Q6_K, norms F32, from random block bytes: every weight_read equals the model filled from the
    reference's dequantisation (q and k un-permuted, norms as f16); without output.weight token_embd is loaded twice"""
    host = load_package().load_host()
    cfg = host.default_config(CODES["q4"], 3)
    cfg.n_vocab, cfg.max_ctx, cfg.n_embd, cfg.n_ffn, cfg.n_layers, cfg.n_heads, cfg.n_kv_heads = 515, 64, 256, 512, 2, 4, 2
    rng = np.random.default_rng(29)
    names = [n for n, _ in convert.tensor_names(cfg.n_layers)]
    back = {convert._gguf_hf_name(g): g for g in ["token_embd.weight", "output_norm.weight", "output.weight"] +
            [f"blk.{i}.{k}.weight" for i in range(cfg.n_layers) for k in convert._GGUF_BLOCK]}
    tensors, want = [], {}
    for name, (rows, cols, dt) in zip(names, cfg.weight_shapes()):
        if name == "lm_head.weight" and not with_output:
            want[name] = want["model.embed_tokens.weight"]
            continue
        if dt == 1:
            w = rng.standard_normal(cols).astype(np.float32)
            tensors.append((back[name], 0, (cols,), w.tobytes()))
            want[name] = convert.to_f16(w.reshape(1, -1))
            continue
        code = 14 if name == "lm_head.weight" else 12
        stream = gguf_ref.random_stream(code, rows, cols, rng, d_max=2e-4)      # (weights of a few hundredths: the logits stay finite)
        n_head = cfg.n_heads if "q_proj" in name else cfg.n_kv_heads if "k_proj" in name else 0
        tensors.append((back[name], code, (rows, cols), stream))
        want[name] = convert.quantize(gguf_ref.dequant(stream, code, rows, cols)[gguf_ref.row_map(rows, n_head)], "q4", "f32")
    path = str(tmp_path / "small.gguf")
    gguf_ref.write_gguf(path, tensors, {"llama.block_count": cfg.n_layers, "llama.attention.head_count": cfg.n_heads,
                                        "llama.attention.head_count_kv": cfg.n_kv_heads})
    a, b = host.model(cfg), host.model(cfg)
    for i, name in enumerate(names):
        a.set_weight(i, want[name])
    b.load_gguf(path)
    same = [np.array_equal(a.weight_read(i), b.weight_read(i)) for i in range(a.n_weights())]
    prompt = rng.integers(0, cfg.n_vocab, 12).astype(np.int32)
    la, lb = a.logits(prompt, 0), b.logits(prompt, 0)
    a.close()
    b.close()
    assert all(same), [names[i] for i, ok in enumerate(same) if not ok]
    assert np.isfinite(la).all() and la.std() > 0 and la.tobytes() == lb.tobytes()
