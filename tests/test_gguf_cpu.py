"""not gpu: the device-free side of GGUF loading: the two new headers against their GGUF_SYMBOLS lists and the
exports, disjoint from every other list and header; convert.open_gguf on tests/gguf_ref.py's writer and its refusals;
gguf_ref.dequant on one hand-written block per format; the command line's --from-gguf on a file that is not there."""
import importlib
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gguf_ref  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402
from test_abi_loads import declared_symbols  # noqa: E402

load_package()
convert = importlib.import_module("tinyllama_cpp_amd.convert")
KV = {"llama.block_count": 1, "llama.attention.head_count": 4, "llama.attention.head_count_kv": 2}


@pytest.mark.parametrize("side, header", [("hipabi.GtenHip", "gten_hip_gguf.h"), ("hostabi.GtenHost", "gten_host_gguf.h")])
def test_gguf_header_is_its_list_exported_and_disjoint(side, header):
    pkg = load_package()
    pkg.build.build_all()
    mod, cls = side.split(".")
    api = getattr(getattr(pkg, mod), cls)()
    names = declared_symbols(header)
    assert names and sorted(api.GGUF_SYMBOLS) == names
    for name in names:
        assert hasattr(api.lib, name), name
    for attr in dir(api):
        if attr.endswith("SYMBOLS") and attr != "GGUF_SYMBOLS":
            assert not set(names) & set(getattr(api, attr)), attr
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != header:
            assert not set(names) & set(declared_symbols(other)), other


def one_layer(skip=(), types=None):
    """the tensors of a 1-layer model, E = 256, F = 512, V = 7: linears Q4_K (or types[name]), norms F32, bytes counting up"""
    types = types or {}
    shapes = {"token_embd": (7, 256), "attn_q": (256, 256), "attn_k": (128, 256), "attn_v": (128, 256), "attn_output": (256, 256),
              "ffn_gate": (512, 256), "ffn_up": (512, 256), "ffn_down": (256, 512), "attn_norm": (256,), "ffn_norm": (256,),
              "output_norm": (256,), "output": (7, 256)}
    out = []
    for k, (key, shape) in enumerate(shapes.items()):
        name = (key if key in ("token_embd", "output_norm", "output") else "blk.0." + key) + ".weight"
        if name in skip:
            continue
        code = types.get(name, 0 if len(shape) == 1 else 12)
        n = 4 * shape[0] if len(shape) == 1 else gguf_ref.src_bytes(code, *shape) if code in gguf_ref.FORMATS else 110 * shape[0]
        out.append((name, code, shape, (np.arange(n) + k).astype(np.uint8)))
    return out


def test_open_gguf_maps_names_shapes_types_and_honours_the_alignment(tmp_path):
    path = str(tmp_path / "m.gguf")
    tensors = one_layer(skip=("output.weight",), types={"blk.0.ffn_down.weight": 14})
    gguf_ref.write_gguf(path, tensors, KV, alignment=64)
    g = convert.open_gguf(path)
    assert (g.n_layers, g.n_head, g.n_head_kv, g.alignment) == (1, 4, 2, 64)
    assert sorted(g.tensors) == sorted(n for n, _ in convert.tensor_names(1))
    for name, code, shape, raw in tensors:
        got, gcode, rows, cols = g[convert._gguf_hf_name(name)]
        assert (gcode, rows, cols) == (code, shape[0] if len(shape) == 2 else 1, shape[-1]) and np.array_equal(got, raw), name
    assert g["lm_head.weight"][0].tobytes() == g["model.embed_tokens.weight"][0].tobytes()          # no output.weight: token_embd twice
    assert g["model.layers.0.mlp.down_proj.weight"][1] == 14
    assert convert.gguf_row_map(8, 2).tolist() == [0, 2, 1, 3, 4, 6, 5, 7] == gguf_ref.row_map(8, 2).tolist()


@pytest.mark.parametrize("kw, tensors, said", [
    ({"magic": b"GGML"}, one_layer(), "not a GGUF file"),
    ({"version": 1}, one_layer(), "version 1 is not supported"),
    ({"version": struct.unpack("<I", struct.pack(">I", 3))[0]}, one_layer(), "big-endian"),
    ({}, one_layer(types={"blk.0.attn_v.weight": 11}), "blk.0.attn_v.weight has ggml type 11"),
    ({}, one_layer(skip=("blk.0.attn_q.weight",)), "tensor blk.0.attn_q.weight is missing"),
])
def test_open_gguf_refuses_by_name(tmp_path, kw, tensors, said):
    path = str(tmp_path / "bad.gguf")
    gguf_ref.write_gguf(path, tensors, KV, **kw)
    with pytest.raises(ValueError, match=said):
        convert.open_gguf(path)


def f16(v):
    return np.array([v], np.float16).view(np.uint8).tolist()


def test_reference_dequant_on_one_hand_written_block_per_format():
    """Q8_0  d 0.5, q[j] = j - 16: x[j] = 0.5 (j - 16)
    Q4_0  d 2, qs[j] = j | (15 - j) << 4: x[j] = 2 (j - 8), x[j + 16] = 2 (7 - j)
    Q5_0  d 1, every nibble 0, qh = bits 0 and 31: x[0] = x[31] = 16 - 16 = 0, every other x = -16
    Q4_K  d 1, dmin 0.5, sc[0] = 3 | 1 << 6, sc[4] = 2, sc[8] = 0x25, qs = 0x21 everywhere: sub-block 0 has s = 3, m = 2 and the low
          nibbles 1: x = 3 * 1 - 0.5 * 2 = 2; sub-block 4 has s = 5 | 1 << 4 = 21, m = 2 | 0: x = 21 - 1 = 20; sub-blocks 1 and 5
          (the high nibbles 2) and all others have s = m = 0: x = 0
    Q5_K  the same with qh[0] = 1, qh[1] = 1 << 4: element 0 of sub-block 0 has q = 17: x = 51 - 1 = 50; element 1 of sub-block 4
          has q = 17: x = 357 - 1 = 356
    Q6_K  d 0.25, ql = 0x53, qh = 0xE4 (the two bits of k are k), sc[0] = 4, sc[1] = -4, sc[4] = 2: k = 0 has q = 3 | 0 << 4, q - 32 =
          -29: x[0..15] = 0.25 * 4 * -29 = -29, x[16..31] = 29; k = 2 takes the high nibble 5 | 2 << 4 = 37: x[64..79] = 0.5 * 5 = 2.5"""
    d = lambda code, b: gguf_ref.dequant(np.array(b, np.uint8), code, 1, gguf_ref.FORMATS[code][2])[0]      # noqa: E731
    j = np.arange(16)
    assert d(8, f16(0.5) + [(q - 16) & 255 for q in range(32)]).tolist() == [0.5 * (q - 16) for q in range(32)]
    assert d(2, f16(2) + (j | (15 - j) << 4).tolist()).tolist() == (2.0 * (j - 8)).tolist() + (2.0 * (7 - j)).tolist()
    assert d(6, f16(1) + [1, 0, 0, 0x80] + [0] * 16).tolist() == [0.0] + [-16.0] * 30 + [0.0]
    sc = [3 | 1 << 6, 0, 0, 0, 2, 0, 0, 0, 0x25, 0, 0, 0]
    want = np.zeros((8, 32))
    want[0], want[4] = 2, 20
    assert d(12, f16(1) + f16(0.5) + sc + [0x21] * 128).tolist() == want.reshape(-1).tolist()
    want[0, 0], want[4, 1] = 50, 356
    assert d(13, f16(1) + f16(0.5) + sc + [1, 16] + [0] * 30 + [0x21] * 128).tolist() == want.reshape(-1).tolist()
    want = np.zeros(256)
    want[:16], want[16:32], want[64:80] = -29, 29, 2.5
    assert d(14, [0x53] * 128 + [0xE4] * 64 + [4, 252, 0, 0, 2] + [0] * 11 + f16(0.25)).tolist() == want.tolist()


def test_cli_from_gguf_on_a_file_that_is_not_there():
    pkg = load_package()
    pkg.build.build_all()
    r = subprocess.run([pkg.build.HOST_CLI, "--from-gguf", "-q4", "--model", "/nonexistent/m.gguf"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "cannot open" in r.stderr, r.stderr[-300:]
