"""not gpu: the device-free side of the LoRA merge: the two new headers against their LORA_SYMBOLS lists and the
exports, disjoint from every other list and header; convert.open_lora on synthetic PEFT adapters; tests/lora_ref.py against
float64 within the bound of a rank-long f32 sum."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from __graft_entry__ import load_package  # noqa: E402
from lora_ref import convert, merge  # noqa: E402
from test_abi_loads import declared_symbols  # noqa: E402


@pytest.mark.parametrize("side, header", [("hipabi.GtenHip", "gten_hip_lora.h"), ("hostabi.GtenHost", "gten_host_lora.h")])
def test_lora_header_is_its_list_exported_and_disjoint(side, header):
    pkg = load_package()
    pkg.build.build_all()
    mod, cls = side.split(".")
    api = getattr(getattr(pkg, mod), cls)()
    names = declared_symbols(header)
    assert names and sorted(api.LORA_SYMBOLS) == names
    for name in names:
        assert hasattr(api.lib, name), name
    for attr in dir(api):
        if attr.endswith("SYMBOLS") and attr != "LORA_SYMBOLS":
            assert not set(names) & set(getattr(api, attr)), attr
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != header:
            assert not set(names) & set(declared_symbols(other)), other


def write_adapter(d, tensors, **cfg):
    from safetensors.numpy import save_file
    os.makedirs(d, exist_ok=True)
    save_file(tensors, os.path.join(d, "adapter_model.safetensors"))
    with open(os.path.join(d, "adapter_config.json"), "w") as f:
        json.dump({"peft_type": "LORA", "r": 4, "lora_alpha": 10, "bias": "none", **cfg}, f)
    return str(d)


def pair(module, r=4, rows=8, cols=32, dtype=np.float16, kind="lora"):
    p = f"base_model.model.{module}.{kind}_"
    return {p + "A.weight": np.full((r, cols), 0.5, dtype), p + "B.weight": np.full((rows, r), 2.0, dtype)}


def test_open_lora_maps_the_keys_and_takes_both_scale_rules(tmp_path):
    tensors = {**pair("model.layers.0.self_attn.q_proj"), **pair("model.layers.1.mlp.down_proj", rows=16, dtype=np.float32)}
    got, scale = convert.open_lora(write_adapter(tmp_path / "a", tensors), n_layers=2)
    assert scale == 2.5 and sorted(got) == ["model.layers.0.self_attn.q_proj.weight", "model.layers.1.mlp.down_proj.weight"]
    a, b = got["model.layers.1.mlp.down_proj.weight"]
    assert a.dtype == np.float32 and a.shape == (4, 32) and b.shape == (16, 4) and (a == 0.5).all() and (b == 2.0).all()
    assert got["model.layers.0.self_attn.q_proj.weight"][0].dtype == np.float16
    d = write_adapter(tmp_path / "b", tensors, use_rslora=True)
    assert convert.open_lora(os.path.join(d, "adapter_model.safetensors"))[1] == 5.0          # the file beside its config


@pytest.mark.parametrize("tensors, cfg, said", [
    (pair("model.embed_tokens", kind="lora_embedding"), {}, "embedding adapter"),
    (pair("model.embed_tokens"), {}, "model.embed_tokens.weight"),
    (pair("lm_head"), {}, "lm_head.weight"),
    (pair("model.layers.0.self_attn.q_proj"), {"modules_to_save": ["lm_head"]}, "modules_to_save"),
    (pair("model.layers.0.self_attn.q_proj"), {"use_dora": True}, "DoRA"),
    (pair("model.layers.0.self_attn.q_proj"), {"bias": "lora_only"}, "bias"),
    (pair("model.layers.0.self_attn.q_proj", r=65), {"r": 65}, "rank 65"),
    (pair("model.layers.5.self_attn.q_proj"), {}, "model.layers.5"),
])
def test_open_lora_refuses_by_name_what_the_merge_cannot_honour(tmp_path, tensors, cfg, said):
    with pytest.raises(ValueError, match=said):
        convert.open_lora(write_adapter(tmp_path / "a", tensors, **cfg), n_layers=2)


@pytest.mark.parametrize("rank", [1, 17, 64])
def test_reference_merge_is_within_the_bound_of_an_f32_sum(rank):
    """a term B A passes through its product, rank - 1 sums (the first, 0 + p, is exact), the multiply by s and the last sum:
    n = rank + 1 roundings at most, so its relative error is at most (1 + u)^n - 1 <= n u / (1 - n u) <= (n + 1) u, u = 2^-24, the
    last step because n (n + 1) u <= 1 (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1); w passes through one"""
    rng = np.random.default_rng(rank)
    w, a, b = (rng.standard_normal(s).astype(np.float32) for s in ((9, 64), (rank, 64), (9, rank)))
    exact = w.astype(np.float64) - 1.75 * (b.astype(np.float64) @ a.astype(np.float64))
    bound = (rank + 2) * 2.0 ** -24 * (np.abs(w) + 1.75 * (np.abs(b).astype(np.float64) @ np.abs(a).astype(np.float64)))
    assert (np.abs(merge(w, a, b, -1.75, "f32", rounded=False) - exact) <= bound).all()
