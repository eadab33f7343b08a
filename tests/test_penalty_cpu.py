"""not gpu: the penalties' restatement (tests/penalty_ref.py) against a plain Python loop, the window arithmetic at its edges, the
new C-ABI headers (include/gten_hip_penalty.h, include/gten_host_penalty.h: exported by the libraries and bound in the Python wrappers),
the host's penalty_ok (host/generate.h) compiled into a small program, and the command line's refusals."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import penalty_ref as ref  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402
from test_abi_loads import declared_symbols  # noqa: E402


def f32(v):
    """v rounded to float32, as a Python float (Python arithmetic on such values, rounded again, is one f32 operation: the double
    result of +, -, * and / of two f32 values rounds to the f32 result -- 53 >= 2 * 24 + 2)"""
    return struct.unpack("f", struct.pack("f", v))[0]


def loop_row(x, ids, r, freq, pres, b=None):
    n = len(x)
    c = [0] * n
    for t in ids:
        if 0 <= t < n:
            c[t] += 1
    out = []
    for i in range(n):
        v = float(x[i])
        if c[i] > 0:
            u = f32(v / f32(r)) if v > 0 else f32(v * f32(r))
            t = f32(f32(float(c[i]) * f32(freq)) + f32(pres))
            v = f32(u - t)
        if b is not None:
            v = f32(v + float(b[i]))
        out.append(v)
    return np.array(out, np.float32)


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def test_the_restatement_against_a_plain_loop():
    g = np.random.default_rng(3)
    for trial in range(40):
        n = int(g.choice([1, 2, 7, 64, 301]))
        x = (g.standard_normal(n) * 4.0).astype(np.float32)
        x[g.integers(0, n)] = 0.0
        if n > 2:
            x[g.integers(0, n)] = -0.0
        ids = g.integers(-2, n + 2, int(g.choice([0, 1, 5, 400]))).tolist()
        r, freq, pres = float(g.choice([0.5, 0.8, 1.0, 1.1, 1.3, 8.0])), float(g.choice([0.0, 0.1, -0.25, 1.5])), float(g.choice([0.0, 0.7, -0.3]))
        b = None
        if trial % 3 == 0:
            b = (g.standard_normal(n) * 2.0).astype(np.float32)
            b[g.integers(0, n)] = -np.inf
        # ((1, 0, 0) in the loop is x / 1 - 0 or x * 1 - 0: the bits of x, so one loop serves both)
        got, want = ref.row(x, ids, r, freq, pres, b), loop_row(x, ids, r, freq, pres, b)
        assert (bits(got) == bits(want)).all(), (trial, n, r, freq, pres)
    # by hand: x = 2, three occurrences, (r, freq, pres) = (2, 0.5, 0.25): 2 / 2 - (3 * 0.5 + 0.25) = -0.75; x = -2: -4 - 1.75
    y = ref.row(np.array([2.0, -2.0, 5.0, 0.0, -0.0], np.float32), [0, 0, 0, 1, 1, 1, 3, 4, 7, -1], 2.0, 0.5, 0.25)
    assert y.tolist()[:3] == [-0.75, -5.75, 5.0] and y[3] == -0.75 and y[4] == -0.75            # (+0 and -0 are "not > 0": 0 * r - t)
    assert ref.counts([0, 0, 5, -1, 6, 2], 6).tolist() == [2, 0, 1, 0, 0, 1]
    # no penalty leaves the bits alone, whatever the window says
    x = np.array([1.5, -0.0, 3.0], np.float32)
    assert (bits(ref.row(x, [0, 1, 2, 2], 1.0, 0.0, 0.0)) == bits(x)).all()
    # a ban stays a ban: the penalty comes first, the table second
    b = np.array([0.0, -np.inf, 1.0], np.float32)
    y = ref.row(np.array([4.0, 9.0, -1.0], np.float32), [1, 1, 2], 0.5, -3.0, 0.0, b)
    assert y[1] == -np.inf and y[0] == 4.0 and y[2] == -0.5 + 3.0 + 1.0


def test_the_window_arithmetic():
    assert ref.window(10, 0, 0) == (0, 10)                              # last_n 0: everything
    assert ref.window(10, 4, 0) == (4, 10)
    assert ref.window(10, 0, 3) == (7, 10)
    assert ref.window(10, 4, 3) == (7, 10) and ref.window(10, 8, 3) == (8, 10)       # n - last_n on either side of start
    assert ref.window(10, 4, 30) == (4, 10) and ref.window(10, 0, 30) == (0, 10)     # n - last_n < 0 <= start
    assert ref.window(10, 12, 0) == (10, 10) and ref.window(10, 12, 5) == (10, 10)   # start > n: nothing
    assert ref.window(0, 0, 0) == (0, 0) and ref.window(1, 0, 1) == (0, 1)
    t = np.arange(100, 120)
    x = np.zeros(200, np.float32) + 1.0
    y = ref.decoder_row(x, t, 10, 2.0, 0.0, 0.0, 4, 3)
    assert np.flatnonzero(y != 1.0).tolist() == [107, 108, 109]
    assert np.flatnonzero(ref.decoder_row(x, t, 10, 2.0, 0.0, 0.0, 12, 0) != 1.0).tolist() == []


def test_penalty_headers_are_exported_and_bound():
    pkg = load_package()
    pkg.build.build_all()
    api = pkg.hipabi.GtenHip()
    names = declared_symbols("gten_hip_penalty.h")
    assert sorted(api.PENALTY_SYMBOLS) == names and len(names) == 4
    for other in ("gten_hip.h", "gten_hip_sample.h", "gten_hip_bias.h", "gten_hip_score.h", "gten_hip_logprobs.h", "gten_hip_nucleus.h"):
        assert not set(names) & set(declared_symbols(other)), other
    for name in names:
        assert hasattr(api.lib, name), name
    host = pkg.hostabi.GtenHost()
    names = declared_symbols("gten_host_penalty.h")
    assert sorted(host.PENALTY_SYMBOLS) == names and len(names) == 7
    for name in names:
        assert hasattr(host.lib, name), name
    header = open(os.path.join(ROOT, "include", "gten_hip_penalty.h")).read()
    assert f"#define GTEN_HIP_PENALTY_HISTORY_MAX {ref.HISTORY_MAX} " in header and api.PENALTY_HISTORY_MAX == ref.HISTORY_MAX
    assert "#define GTEN_HIP_PENALTY_R_MIN 0.125f\n" in header and "#define GTEN_HIP_PENALTY_R_MAX 8.0f\n" in header
    assert "#define GTEN_HIP_PENALTY_ADD_MAX 100.0f\n" in header
    # the penalty lives in its own array: the sampler's request record and the cut keep their layouts
    csrc = os.path.join(ROOT, "tinyllama.cpp_amd", "csrc")
    assert "struct PenParam" in open(os.path.join(csrc, "gten_decode_penalty.h")).read()
    assert "PenParam" not in open(os.path.join(csrc, "gten_decode_sample.h")).read()
    assert "PenParam" not in open(os.path.join(csrc, "gten_decode_nucleus.h")).read()
    assert ctypes_size(pkg.hostabi.HostPenalties) == 5 * 8 + 5 * 4 + 4                # gten_host_penalties on LP64


def ctypes_size(t):
    import ctypes
    return ctypes.sizeof(t)


PENALTY_OK_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "host/generate.h"
int main(int argc, char** argv)
{
    for (int i = 1; i + 3 < argc; i += 4)
        std::printf("%d\n", gten::penalty_ok(std::strtof(argv[i], nullptr), std::strtof(argv[i + 1], nullptr), std::strtof(argv[i + 2], nullptr),
                                             std::atoi(argv[i + 3])) ? 1 : 0);
    gten::Request r;
    r.rep = 1.f; std::printf("%d\n", r.penalises() ? 1 : 0);
    r.pres = -0.5f;
    const int with_prompt = r.start(7);
    r.count_prompt = false;
    std::printf("%d %d %d\n", r.penalises() ? 1 : 0, with_prompt, r.start(7));
    return 0;
}
"""


def test_host_penalty_ok_edges(tmp_path):
    """host/generate.h's check, compiled alone (the header names the device library only inside templates nobody instantiates here)"""
    src, exe = tmp_path / "penalty_ok.cpp", tmp_path / "penalty_ok"
    src.write_text(PENALTY_OK_MAIN)
    pkg_dir = os.path.join(ROOT, "tinyllama.cpp_amd")
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-fopenmp", "-I" + os.path.join(ROOT, "include"), "-I" + pkg_dir, "-o", str(exe), str(src),
                        "-L" + os.path.join(pkg_dir, "csrc"), "-lgten_hip", "-Wl,-rpath," + os.path.join(pkg_dir, "csrc")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = [((1, 0, 0, 0), 1), ((0.125, 100, -100, 0), 1), ((8, 0, 0, 5), 1), ((0.1249, 0, 0, 0), 0), ((8.001, 0, 0, 0), 0), (("nan", 0, 0, 0), 0),
             (("inf", 0, 0, 0), 0), ((0, 0, 0, 0), 0), ((-1.1, 0, 0, 0), 0), ((1.1, 100.5, 0, 0), 0), ((1.1, 0, -100.5, 0), 0), ((1.1, "nan", 0, 0), 0),
             ((1.1, 0, "inf", 0), 0), ((1.1, 0, 0, -1), 0), ((1.1, -3.5, 2.5, 64), 1)]
    args = [str(v) for c, _ in cases for v in c]
    out = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split("\n")
    assert [int(v) for v in lines[: len(cases)]] == [w for _, w in cases]
    assert [ref.penalty_ok(float(c[0]), float(c[1]), float(c[2]), 0, int(c[3])) for c, _ in cases] == [bool(w) for _, w in cases]
    assert lines[len(cases)] == "0" and lines[len(cases) + 1] == "1 0 7"


@pytest.fixture(scope="module")
def cli():
    pkg = load_package()
    pkg.build.build_all()
    return pkg.build.HOST_CLI


def run(cli, *args):
    return subprocess.run([cli, *args], capture_output=True, text=True, timeout=120)


def test_cli_parses_and_refuses_the_penalty_flags(cli):
    """every refusal comes from the option parser, before a checkpoint is opened"""
    for args, said in ((("--repeat-penalty", "0"), "repeat-penalty must be"), (("--repeat-penalty", "0.12"), "repeat-penalty must be"),
                       (("--repeat-penalty", "8.5"), "repeat-penalty must be"), (("--repeat-penalty", "-1.1"), "repeat-penalty must be"),
                       (("--repeat-penalty", "abc"), "Invalid repeat-penalty value"), (("--repeat-penalty", "1.1x"), "Invalid repeat-penalty value"),
                       (("--repeat-penalty", "nan"), "Invalid repeat-penalty value"), (("--repeat-penalty",), "value is missing"),
                       (("--frequency-penalty", "101"), "frequency-penalty must be"), (("--frequency-penalty", "inf"), "Invalid frequency-penalty value"),
                       (("--frequency-penalty", ""), "Invalid frequency-penalty value"), (("--presence-penalty", "-100.5"), "presence-penalty must be"),
                       (("--presence-penalty", "x"), "Invalid presence-penalty value"), (("--presence-penalty",), "value is missing"),
                       (("--repeat-last-n", "-1"), "repeat-last-n must be"), (("--repeat-last-n", "4.5"), "Invalid repeat-last-n value"),
                       (("--repeat-last-n", "x"), "Invalid repeat-last-n value"), (("--repeat-last-n",), "value is missing"),
                       (("--repeat-penalty", "1.1", "--score", "/nonexistent/text"), "do not apply to --score")):
        r = run(cli, *args)
        assert r.returncode != 0 and said in r.stderr and "cannot open" not in r.stderr, (args, r.stderr[-300:])
    r = run(cli, "--help")
    assert r.returncode == 0 and all(f in r.stdout for f in ("--repeat-penalty", "--frequency-penalty", "--presence-penalty", "--repeat-last-n"))
    # well-formed requests pass the parser, with -greedy too and beside the other stages: the next complaint is the missing checkpoint
    for args in (("--repeat-penalty", "1.1"), ("--repeat-penalty", "0.125"), ("--repeat-penalty", "8"), ("-greedy", "--repeat-penalty", "1.3"),
                 ("--frequency-penalty", "-0.5", "--presence-penalty", "100", "--repeat-last-n", "64"), ("-greedy", "--presence-penalty", "0.5"),
                 ("--repeat-penalty", "1.1", "--top-p", "0.9", "--logprobs", "3", "--ban", "2,0", "--min-new", "3"), ("--repeat-last-n", "0")):
        r = run(cli, *args, "--model", "/nonexistent/m.gten")
        assert r.returncode != 0 and "cannot open the checkpoint" in r.stderr, (args, r.stderr[-300:])
