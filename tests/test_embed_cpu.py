"""not gpu: the embedding calls' device-free side.  The plan (host/embed_plan.h, exported as gten_host_embed_plan)
against its restatement in tests/embed_ref.py over a grid of length lists; the plan header alone under ASan + UBSan
(tests/host_embed_plan.cpp, a stand-alone program); the numpy reference against plain float64 pooling, within the bound of the stated
summation; the symbols of include/gten_hip_embed.h and include/gten_host_embed.h exported and bound."""
import itertools
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import embed_ref as ref  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402


def host():
    pkg = load_package()
    pkg.build.build_all()
    return pkg.hostabi.GtenHost()


def test_plan_agrees_with_its_restatement_over_a_grid():
    h = host()
    n = 0
    lens = (1, 15, 16, 17, 128, 129, 2047, 2048, 2049)
    lists = [list(c) for k in (1, 2, 3) for c in itertools.product(lens, repeat=k)]
    for count in (31, 32, 33, 65):                                   # a 33rd text; the 4096-row edge: 32 x 128 fits, one more row does not
        for length in (9, 16, 127, 128, 129, 2048):
            lists.append([length] * count)
    lists.append([128] * 31 + [129])
    lists.append([128] * 31 + [127, 16])
    lists.append([2048, 2048, 1, 16])
    lists.append([2048, 2047, 15, 16, 1, 2048])
    rng = np.random.default_rng(5)
    for _ in range(50):
        lists.append([int(x) for x in rng.integers(1, 400, rng.integers(1, 120))])
    for lengths in lists:
        for seg_ok in (0, 1):
            assert h.embed_plan(lengths, seg_ok) == ref.plan(lengths, seg_ok), (lengths, seg_ok)
            n += 1
    assert n > 1500
    assert h.embed_plan([20, 5, 30]) == ([0, 1, 0], [0, 1])         # a text that goes alone does not close the open group
    assert h.embed_plan([16] * 33) == ([0] * 32 + [1], [0, 0])
    assert h.embed_plan([128] * 32) == ([0] * 32, [0])
    assert h.embed_plan([128] * 31 + [129]) == ([0] * 31 + [1], [0, 0])
    assert h.embed_plan([20, 30], False) == ([0, 1], [1, 1])
    assert h.embed_plan([]) is None and h.embed_plan([4, 0]) is None and h.embed_plan([-3]) is None


def test_embed_plan_under_sanitizers(tmp_path):
    """the plan over length lists with exactly sized outputs and its invariants (tests/host_embed_plan.cpp), under ASan + UBSan.  The
    program includes host/embed_plan.h alone, and that header is device-free."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = os.path.join(ROOT, "tests", "host_embed_plan.cpp")
    includes = [line for line in open(src) if line.startswith("#include \"")]
    assert includes == ['#include "../tinyllama.cpp_amd/host/embed_plan.h"\n'], includes
    plan = open(os.path.join(ROOT, "tinyllama.cpp_amd", "host", "embed_plan.h")).read()
    assert "#include" not in plan and "gten_hip_" not in plan.replace("gten_hip_row_segments_ok", "")   # device-free: not even the standard library
    exe = str(tmp_path / "host_embed_plan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           src, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:protect_shadow_gap=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    assert "host_embed_plan ok" in r.stdout


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 128, 129, 700, 2048])
def test_reference_against_float64_pooling(n):
    """embed_ref's mean is the stated summation: at most 63 additions inside a chunk, ceil(n / 64) - 1 across chunks and one division, each
    within 2^-24 relative of an exact result whose magnitude never passes sum_r |x[r][c]|.  Normalised vectors have norm 1 within 2^-22."""
    rng = np.random.default_rng(n)
    for dtype, n_embd in ((ref.F16, 96), (ref.Q8, 64)):
        if dtype == ref.F16:
            rows = (rng.standard_normal((n, n_embd)) * rng.choice([1e-3, 1.0, 300.0])).astype(np.float16).view(np.uint8).reshape(n, -1)
        else:
            rows = ref.pack_q8(rng.integers(-127, 128, (n, n_embd)), rng.uniform(0.0, 0.1, (n, n_embd // 32)).astype(np.float16))
        assert rows.shape == (n, ref.row_bytes(dtype, n_embd))
        x = ref.rows_to_f32(rows, dtype)
        x64 = x.astype(np.float64)
        m = ref.pool(x, "mean", False)
        assert m.dtype == np.float32
        bound = (63 + math.ceil(n / 64) + 1) * 2.0 ** -24 * np.abs(x64).sum(axis=0) / n
        err = np.abs(m.astype(np.float64) - x64.mean(axis=0))
        assert (err <= bound).all(), (dtype, float((err - bound).max()))
        assert np.array_equal(ref.pool(x, "last", False), x[-1])
        for pooling in ("mean", "last"):
            e = ref.pool(x, pooling, True)
            assert e.dtype == np.float32
            norm = math.sqrt(float((e.astype(np.float64) ** 2).sum()))
            assert abs(norm - 1.0) <= 2.0 ** -22, (dtype, pooling, norm)
    # a row of zeros stays zero (no NaN), -0 survives a mean of -0 rows and a sum that starts from its first term
    z = np.zeros((5, 64), np.float32)
    assert np.array_equal(ref.pool(z, "mean", True), np.zeros(64, np.float32)) and not np.signbit(ref.pool(z, "mean", True)).any()
    assert np.signbit(ref.pool(-z, "mean", False)).all() and not np.signbit(ref.pool(-z, "mean", True)).any()
    assert ref.ulps(np.float32([1.0, -0.0]), np.float32([np.nextafter(np.float32(1), np.float32(2)), 0.0])).tolist() == [1, 0]


def test_oracle_with_an_identity_head_returns_the_row(oracle):
    """what tests/test_embed_gpu.py's comparison of hidden rows with the oracle rests on: with an lm_head whose first n_embd rows are the
    identity in the weight dtype, the oracle's matmul_2d gives the input row times q * f16(delta) of a quantised 1 -- exactly in f16 mode
    (a one-hot dot product), and in q8 / q4 without requantising the Q8 row it reads (the same bits as dequantise, then one f32 multiply)"""
    from helpers import F32, MODES, act_rows, rng
    E, V = 256, 512
    eye = np.zeros((V, E), np.float32)
    eye[:E] = np.eye(E, dtype=np.float32)
    consts = {"f16": 1.0, "q8": 127 * float(np.float16(1 / 127)), "q4": 7 * float(np.float16(1 / 7))}
    for name, wd, ad in MODES():
        w = oracle.quantize_weight(eye, wd)
        c = np.float32(consts[name])
        assert np.array_equal(oracle.dequantize_rows(w, wd, E), eye * c)
        xb, xf = act_rows(oracle, rng(3), 6, E, ad, 1.0)
        assert np.array_equal(xf, ref.rows_to_f32(xb, ad))
        out = np.zeros((6, V * 4), np.uint8)
        oracle.matmul_2d(xb, ad, w, wd, out, F32, 6, E, V, 0)
        got = out.view(np.float32).reshape(6, V)
        assert (got[:, E:] == 0).all()
        assert np.array_equal(got[:, :E], np.multiply(xf, c, dtype=np.float32)), name


def test_command_line_refuses_embed_with_generation_flags(tmp_path):
    """--embed and its flags: what needs no GPU.  The option checks run before any file is opened."""
    pkg = load_package()
    pkg.build.build_all()
    cli = pkg.build.HOST_CLI

    def run(*args):
        return subprocess.run([cli, *args], capture_output=True, text=True, timeout=60)
    texts = str(tmp_path / "texts.txt")
    open(texts, "w").write("one text\nanother\n")
    for extra in (["-greedy"], ["-p", "hi"], ["--npred", "5"], ["--temp", "0.5"], ["--topk", "4"], ["--seed", "3"], ["--ids"], ["--top-p", "0.5"],
                  ["--repeat-penalty", "1.1"], ["--ban", "5"], ["--logprobs", "2"], ["--stop", "7"], ["--regex", "a+"], ["--stop-text", "x"],
                  ["--ctx-shift", "4"], ["--score", texts]):
        r = run("--embed", texts, *extra)
        assert r.returncode != 0 and "--embed does not generate" in r.stderr, (extra, r.stderr[-300:])
    for alone in (["--pooling", "last"], ["--no-normalize"], ["--layer", "3"]):
        r = run(*alone)
        assert r.returncode != 0 and "need --embed" in r.stderr, alone
    assert run("--embed", texts, "--pooling", "max").returncode != 0
    assert run("--embed", texts, "--layer", "23").returncode != 0 and run("--embed", texts, "--layer", "-1").returncode != 0
    assert run("--embed").returncode != 0
    r = run("-q4", "--embed", texts, "--pooling", "last", "--no-normalize", "--layer", "5", "--model", str(tmp_path / "nope.gten"))
    assert r.returncode != 0 and "cannot open the checkpoint" in r.stderr          # accepted as far as the options go
    h = run("--help").stdout
    assert "--embed FILE" in h and "--pooling mean|last" in h and "--no-normalize" in h and "--layer N" in h


def declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gten_(?:hip|host)_[a-z0-9_]+)\s*\(", text)))


def test_new_headers_are_exported_and_bound():
    pkg = load_package()
    pkg.build.build_all()
    api, h = pkg.hipabi.GtenHip(), pkg.hostabi.GtenHost()
    names = declared("gten_hip_embed.h")
    assert names == ["gten_hip_pool_rows"] == sorted(api.EMBED_SYMBOLS)
    for name in names:
        assert hasattr(api.lib, name), f"{name} declared in include/gten_hip_embed.h but not exported"
    names = declared("gten_host_embed.h")
    assert len(names) == 4 and names == sorted(h.EMBED_SYMBOLS)
    for name in names:
        assert hasattr(h.lib, name), f"{name} declared in include/gten_host_embed.h but not exported"
    assert api.POOLINGS == h.POOLINGS == {"mean": 0, "last": 1}
    # the two headers whose symbol lists tests/test_abi_loads.py pins did not grow by them
    for header in ("gten_hip.h", "gten_host.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert "embed_many" not in text and "pool_rows" not in text
    # host/capi.cpp and the headers it instantiates go on linking against the stand-in of include/gten_hip.h alone: the one translation
    # unit of the library that names the device entry point is host/capi_embed.cpp, through host/embed.h; the kernels live in the operator
    # unit, not the decoder's
    hostdir = os.path.join(ROOT, "tinyllama.cpp_amd", "host")
    for f in sorted(os.listdir(hostdir)):
        if f.endswith((".h", ".cpp")) and f not in ("capi_embed.cpp", "embed.h", "tinyllama_cli.cpp"):
            text = open(os.path.join(hostdir, f)).read()
            assert "gten_hip_pool_rows" not in text and "gten_hip_embed.h" not in text and '#include "embed.h"' not in text, f
    csrc = os.path.join(ROOT, "tinyllama.cpp_amd", "csrc")
    users = sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".h")) and "gten_pool_rows.h" in open(os.path.join(csrc, f)).read())
    assert users == ["gten_ops.hip", "gten_pool_rows.h"], users
