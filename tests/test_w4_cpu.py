"""not gpu: the device-free side of GPTQ / AWQ loading: the two new headers against their W4_SYMBOLS lists and the
exports, disjoint from every other list and header; convert.open_quantized on synthetic safetensors files and its refusals;
w4_ref.dequant on one hand-written group per layout."""
import importlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import w4_ref  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402
from test_abi_loads import declared_symbols  # noqa: E402

load_package()
convert = importlib.import_module("tinyllama_cpp_amd.convert")


@pytest.mark.parametrize("side, header", [("hipabi.GtenHip", "gten_hip_w4.h"), ("hostabi.GtenHost", "gten_host_w4.h")])
def test_w4_header_is_its_list_exported_and_disjoint(side, header):
    pkg = load_package()
    pkg.build.build_all()
    mod, cls = side.split(".")
    api = getattr(getattr(pkg, mod), cls)()
    names = declared_symbols(header)
    assert names and sorted(api.W4_SYMBOLS) == names
    for name in names:
        assert hasattr(api.lib, name), name
    for attr in dir(api):
        if attr.endswith("SYMBOLS") and attr != "W4_SYMBOLS":
            assert not set(names) & set(getattr(api, attr)), attr
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != header:
            assert not set(names) & set(declared_symbols(other)), other


def write_checkpoint(d, layout, qc, skip=(), g_idx=None, config="config.json"):
    """a 1-layer checkpoint, E = 32, F = 64, V = 7, group 32: random 4-bit linears, f16 dense tensors, `qc` as its settings"""
    from safetensors.numpy import save_file
    rng = np.random.default_rng(3)
    shapes = {"self_attn.q_proj": (32, 32), "self_attn.k_proj": (16, 32), "self_attn.v_proj": (16, 32), "self_attn.o_proj": (32, 32),
              "mlp.gate_proj": (64, 32), "mlp.up_proj": (64, 32), "mlp.down_proj": (32, 64)}
    tensors = {"model.embed_tokens.weight": np.ones((7, 32), np.float16), "lm_head.weight": np.ones((7, 32), np.float16), "model.norm.weight": np.ones(32, np.float16),
               "model.layers.0.input_layernorm.weight": np.ones(32, np.float16), "model.layers.0.post_attention_layernorm.weight": np.ones(32, np.float16)}
    for key, (n, k) in shapes.items():
        parts = dict(zip(("qweight", "qzeros", "scales"), w4_ref.random_source(layout, n, k, 32, rng)))
        if g_idx is not None:
            parts["g_idx"] = (np.arange(k) // 32).astype(np.int32) if g_idx == "trivial" else (np.arange(k)[::-1] // 32).astype(np.int32)
        tensors.update({f"model.layers.0.{key}.{part}": a for part, a in parts.items()})
    save_file({k: v for k, v in tensors.items() if k not in skip}, os.path.join(d, "model.safetensors"))
    with open(os.path.join(d, config), "w") as f:
        json.dump({"quantization_config": qc} if config == "config.json" else qc, f)
    return tensors


@pytest.mark.parametrize("layout, qc, config, g_idx, zero_offset", [
    ("gptq", {"quant_method": "gptq", "bits": 4, "group_size": 32, "desc_act": False, "sym": True}, "config.json", "trivial", 1),
    ("gptq", {"bits": 4, "group_size": 32, "desc_act": True, "sym": False, "checkpoint_format": "gptq_v2"}, "quantize_config.json", "reversed", 0),
    ("awq", {"quant_method": "awq", "bits": 4, "group_size": 32, "version": "GEMM", "zero_point": True}, "config.json", None, 0),
])
def test_open_quantized_reads_the_settings_the_tensors_and_whether_g_idx_is_trivial(tmp_path, layout, qc, config, g_idx, zero_offset):
    tensors = write_checkpoint(str(tmp_path), layout, qc, g_idx=g_idx, config=config)
    ck = convert.open_quantized(str(tmp_path / "model.safetensors") if layout == "awq" else str(tmp_path))      # a file | a directory
    assert (ck.layout, ck.zero_offset, ck.group_size, ck.n_layers) == (layout, zero_offset, 32, 1)
    name = "model.layers.0.mlp.down_proj.weight"
    assert ck.is_quantized(name) and not ck.is_quantized("lm_head.weight") and not ck.is_quantized("model.layers.0.input_layernorm.weight")
    qweight, qzeros, scales, got_g, rows, cols = ck.linear(name)
    assert (rows, cols) == (32, 64) and np.array_equal(qweight, tensors[name[:-6] + "qweight"]) and np.array_equal(scales, tensors[name[:-6] + "scales"])
    assert ck.trivial_g_idx == ({} if g_idx is None else {name: g_idx == "trivial"})
    assert (got_g is None) == (g_idx != "reversed") and (got_g is None or got_g.tolist() == [1] * 32 + [0] * 32)
    assert ck.dense("model.norm.weight")[1] == "f16"


@pytest.mark.parametrize("layout, change, skip, said", [
    ("gptq", {"bits": 8}, (), "8-bit weights are not supported"),
    ("gptq", {"group_size": 48}, (), "group_size 48 is not supported"),
    ("gptq", {"checkpoint_format": "marlin"}, (), "checkpoint_format 'marlin' is a repacked form"),
    ("awq", {"version": "gemv"}, (), "AWQ version 'gemv' is not supported"),
    ("awq", {"quant_method": "bitsandbytes"}, (), "quant_method 'bitsandbytes' is not supported"),
    ("awq", {}, ("model.layers.0.mlp.up_proj.scales",), "the tensor model.layers.0.mlp.up_proj.scales is missing"),
])
def test_open_quantized_refuses_by_name(tmp_path, layout, change, skip, said):
    write_checkpoint(str(tmp_path), layout, dict({"quant_method": layout, "bits": 4, "group_size": 32, "version": "gemm"}, **change), skip=skip)
    with pytest.raises(ValueError, match=said):
        convert.open_quantized(str(tmp_path))


def test_reference_dequant_on_one_hand_written_group_per_layout():
    """N = 8, K = 32, one group.
    gptq  every qweight word 0x76543210: q(k, n) = k & 7.  qzeros 0xF6543210: the stored zero of column n is n, 15 for column 7; with
          zero_offset 1 z = n + 1, and 16 -- no wrap -- for column 7.  scales 0.5, column 1: 2.
          D(0, k) = 0.5 ((k & 7) - 1), D(1, k) = 2 ((k & 7) - 2), D(7, k) = 0.5 ((k & 7) - 16); with zero_offset 0 D(7, k) = 0.5 ((k & 7) - 15)
    awq   every qweight word 0x76543210 (nibble position p holds p), row 5: 0.  Column j sits at position P[j], so q(k, j) = P[j] =
          0, 4, 1, 5, 2, 6, 3, 7 and q(5, j) = 0.  qzeros 0x00000010: position 1 is column 2 (P[2] = 1), so z(2) = 1, the others 0.
          scales 0.25: D(n, k) = 0.25 (P[n] - [n = 2]), D(n, 5) = -0.25 [n = 2]"""
    word = lambda v, shape: np.full(shape, v, np.uint32).view(np.int32)      # noqa: E731
    k7 = np.arange(32) & 7
    scales = np.full((1, 8), 0.5, np.float16)
    scales[0, 1] = 2
    d = w4_ref.dequant("gptq", word(0x76543210, (4, 8)), word(0xF6543210, (1, 1)), scales, None, 1, 32)
    assert d.shape == (8, 32) and d[0].tolist() == (0.5 * (k7 - 1)).tolist() and d[1].tolist() == (2.0 * (k7 - 2)).tolist() and d[7].tolist() == (0.5 * (k7 - 16)).tolist()
    assert w4_ref.dequant("gptq", word(0x76543210, (4, 8)), word(0xF6543210, (1, 1)), scales, np.zeros(32, np.int32), 0, -1)[7].tolist() == (0.5 * (k7 - 15)).tolist()
    qweight = word(0x76543210, (32, 1))
    qweight[5] = 0
    d = w4_ref.dequant("awq", qweight, word(0x00000010, (1, 1)), np.full((1, 8), 0.25, np.float16), None, 0, 32)
    want = np.repeat((0.25 * (w4_ref.P - (np.arange(8) == 2)))[:, None], 32, axis=1)
    want[:, 5] = -0.25 * (np.arange(8) == 2)
    assert d.tolist() == want.tolist()
