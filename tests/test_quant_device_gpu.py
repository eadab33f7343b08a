"""-m gpu: weights quantised and packed on the device (include/gten_hip_quant.h) against the converter
(tinyllama.cpp_amd/convert.py), byte for byte: gten_hip_quantize_weight == gten_hip_pack_weight(convert.quantize(...)) for every
source and destination dtype on matrices with the awkward blocks planted; the refusals; a small model loaded both ways; the
command line's --from-f16."""
import importlib
import subprocess

import numpy as np
import pytest

from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from test_cli_gpu import write_vocab

pytestmark = pytest.mark.gpu

load_package()
convert = importlib.import_module("tinyllama_cpp_amd.convert")
CODES = {"f16": 1, "q8": 3, "q4": 4}
SHAPES = [(1, 32), (3, 96), (5, 32 * 17), (65, 2048)]     # one block | fewer blocks than a wave | a tail group | rows > a wave, full rows


def as_src(w, src):
    """f32 values already rounded to `src` -> the elements as the device takes them"""
    return {"f32": lambda: w, "f16": lambda: w.astype(np.float16), "bf16": lambda: (w.view(np.uint32) >> 16).astype(np.uint16)}[src]()


def planted(src, qmax, rng):
    """the blocks of the issue: zeros; one non-zero element; x * scale on k + 0.5 for even and odd k (delta = 2^-6 exactly);
    a subnormal f16 delta (2^-20); a delta that underflows to 0 in f16; f32: an infinite f16 delta (2^17); f16: a subnormal
    delta that rint(x * scale) leaves int8 under (q8: 300 / 2 = 150; q4: 10 / 1 + 7 = 17 spills over its nibble)"""
    n = lambda hi: rng.integers(-hi, hi + 1, 32).astype(np.float32)
    one = np.zeros(32, np.float32)
    one[19] = -0.375
    ties = n(qmax) / 64
    ties[[0, 1, 2, 3, 4, 17, 18, 19, 20]] = np.array([qmax, 0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, 4.5], np.float32) / 64
    sub = n(qmax * 4) * 2.0 ** -22
    sub[5] = qmax * 2.0 ** -20
    if src == "f16":
        under = rng.integers(-3, 4, 32).astype(np.float32) * 2.0 ** -24
        under[30] = 3 * 2.0 ** -24
        top = 300 if qmax == 127 else 10
        last = n(top) * 2.0 ** -24
        last[[2, 21]] = np.array([top, -top], np.float32) * 2.0 ** -24
    else:
        under = n(qmax) * 2.0 ** -30
        under[30] = qmax * 2.0 ** -30
        last = n(qmax) * 2.0 ** 17 if src == "f32" else n(qmax)
        last[11] = qmax * 2.0 ** (17 if src == "f32" else 0)
    return [np.zeros(32, np.float32), one, ties, sub, under, last]


def matrix(src, dst, rows, cols):
    rng = np.random.default_rng(rows * 4099 + cols)
    w = (rng.standard_normal((rows, cols)) * 0.05).astype(np.float32)
    blocks = w.reshape(-1, 32)
    if dst != "f16":
        for i, b in enumerate(planted(src, 127 if dst == "q8" else 7, rng)[: len(blocks) - 1]):
            blocks[len(blocks) - 1 - i] = b              # from the end: (1, 32) keeps its one ordinary block
    elif src != "f16":                                   # f16 destination: overflow to infinity, both ties at the ends, underflow
        blocks[-1][:7] = [1e6, -65520.0, 65519.0, 2.0 ** -25, 3 * 2.0 ** -25, -1e-8, 6.1e-5]
    with np.errstate(over="ignore"):
        return convert._round_to(w, src)


@pytest.mark.parametrize("rows, cols", SHAPES)
@pytest.mark.parametrize("dst", ["q8", "q4", "f16"])
@pytest.mark.parametrize("src", ["f32", "bf16", "f16"])
def test_quantize_weight_is_pack_of_the_converter(hip, src, dst, rows, cols):
    w = matrix(src, dst, rows, cols)
    want_buf = hip.upload_weight(convert.quantize(w, dst, src), CODES[dst], rows, cols)
    got_buf = hip.quantize_weight(as_src(w, src), src, CODES[dst], rows, cols)
    want, got = want_buf.download(), got_buf.download()
    want_buf.free()
    got_buf.free()
    assert got.size == rows * hip.row_bytes(CODES[dst], cols)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("dst", ["q8", "q4", "f16"])
@pytest.mark.parametrize("src", ["f32", "bf16", "f16"])
def test_quantize_weight_refuses_non_finite_input_and_ragged_rows(hip, src, dst):
    Err = load_package().hipabi.GtenHipError
    for bad, at in ((np.nan, (2, 70)), (np.inf, (0, 0)), (-np.inf, (4, 32 * 17 - 1))):
        w = matrix(src, dst, 5, 32 * 17)
        w[at] = bad
        with pytest.raises(Err, match="quantize_weight.*NaN or an infinity"):
            hip.quantize_weight(as_src(w, src), src, CODES[dst], 5, 32 * 17)
    w = convert._round_to(np.linspace(-2.0, 6e4 if src == "f16" else 7e4, 3 * 47, dtype=np.float32).reshape(3, 47), src)
    if dst == "f16":                 # any width, here one whose last lane takes a tail of 5 (and the flag of the calls above is down again)
        got = hip.quantize_weight(as_src(w, src), src, CODES[dst], 3, 47)
        assert got.download().tobytes() == convert.to_f16(w).tobytes()
        got.free()
    else:
        w = np.full((3, 48), 0.25, np.float32)
        with pytest.raises(Err, match="quantize_weight: cols 48"):
            hip.quantize_weight(as_src(w, src), src, CODES[dst], 3, 48)


def small_model(host, wd):
    cfg = host.default_config(CODES[wd], 3)
    cfg.n_vocab, cfg.max_ctx, cfg.n_embd, cfg.n_ffn, cfg.n_layers, cfg.n_heads, cfg.n_kv_heads = 515, 64, 256, 512, 2, 4, 2
    return cfg


@pytest.mark.parametrize("wd", ["q4", "q8"])
def test_a_model_loaded_from_the_f16_file_is_the_converted_model(hip, tmp_path, wd):
    host = load_package().load_host()
    cfg = small_model(host, wd)
    rng = np.random.default_rng(77)
    ws = [convert._round_to((rng.standard_normal((r, c)) * (0.05 if r > 1 else 1.0)).astype(np.float32), "f16") for r, c, _ in cfg.weight_shapes()]
    names = [n for n, _ in convert.tensor_names(cfg.n_layers)]
    path = str(tmp_path / "small.f16.gten")
    convert.write_gten(path, lambda name: ws[names.index(name)], cfg.n_layers, "f16")
    a, b = host.model(cfg), host.model(cfg)
    for i, (w, (_, _, dt)) in enumerate(zip(ws, cfg.weight_shapes())):
        a.set_weight(i, convert.quantize(w, "f16" if dt == 1 else wd, "f16"))
    b.load_gten_f16(path)
    for i in range(a.n_weights()):
        assert np.array_equal(a.weight_read(i), b.weight_read(i)), i
    prompt = rng.integers(0, cfg.n_vocab, 20).astype(np.int32)
    la, lb = a.logits(prompt, 0), b.logits(prompt, 0)
    a.close()
    b.close()
    assert np.isfinite(la).all() and la.std() > 0 and la.tobytes() == lb.tobytes()


def test_cli_from_f16_prints_the_ids_of_the_converted_file(hip, tmp_path):
    """the command line builds the full-size model: a synthetic f16 file, and the q4 file the converter makes of its records"""
    pkg = load_package()
    host = pkg.load_host()
    cfg = host.default_config(1, 1)
    f16, q4, vocab = str(tmp_path / "m.f16.gten"), str(tmp_path / "m.q4.gten"), str(tmp_path / "vocab.bin")
    host.write_gten(cfg, 99, f16)
    write_vocab(vocab)
    shapes = iter(cfg.weight_shapes())
    with open(f16, "rb") as f:
        f.seek(8)

        def record(name):
            rows, cols, _ = next(shapes)
            f.seek(2 * (4 + len(name.encode())) + 4, 1)
            return np.fromfile(f, np.float16, rows * cols).astype(np.float32).reshape(rows, cols), "f16"
        convert.write_gten(q4, record, cfg.n_layers, "q4")
    runs = [subprocess.run([pkg.build.HOST_CLI, "-q4", *extra, "-greedy", "--ids", "--npred", "24", "--model", path, "--tokenizer", vocab,
                            "-p", "hello world"], capture_output=True, text=True, timeout=300) for extra, path in (([], q4), (["--from-f16"], f16))]
    for r in runs:
        assert r.returncode == 0, r.stderr[-2000:]
    assert runs[0].stdout.split() == runs[1].stdout.split() and len(runs[0].stdout.split()) > 0
    wrong = subprocess.run([pkg.build.HOST_CLI, "-q4", "--model", f16, "--tokenizer", vocab, "-p", "x"], capture_output=True, text=True, timeout=300)
    assert wrong.returncode != 0 and "does not match the expected size" in wrong.stderr
