"""not gpu: Mirostat v2's device-free side.  The shared arithmetic (csrc/gten_miro_math.h, exported as
gten_hip_miro_lg16_host / _update_host / _q16_host) against the restatement in Python integers (tests/miro_ref.py); the header alone under
ASan + UBSan (tests/host_miro_math.cpp, a stand-alone program); the input condition of tests/test_mirostat_gpu.py's operator test and
the feedback property, both from the restatement alone; the symbols of include/gten_hip_mirostat.h exported and bound."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mirostat_cases as cases  # noqa: E402
import miro_ref as ref  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402
from test_abi_loads import declared_symbols  # noqa: E402


@pytest.fixture(scope="module")
def api():
    pkg = load_package()
    pkg.build.build_all()
    return pkg.hipabi.GtenHip()


def lg16_values():
    """1, 2, 3; 2^k - 1, 2^k, 2^k + 1 for k up to 52; 2^36; 2^52 - 1; 10^5 random values"""
    v = {1, 2, 3, 1 << 36, (1 << 52) - 1}
    for k in range(1, 53):
        v |= {(1 << k) - 1, 1 << k, (1 << k) + 1}
    r = np.random.default_rng(16)
    v |= {int(x) for x in r.integers(1, 1 << 52, 80000)}
    e = r.integers(0, 53, 20000).astype(np.uint64)                                   # ... a fifth of them log-uniform: every exponent occurs
    v |= {int(x) for x in ((np.uint64(1) << e) | (r.integers(0, 1 << 62, 20000).astype(np.uint64) & ((np.uint64(1) << e) - np.uint64(1))))}
    return sorted(x for x in v if x >= 1)


def test_lg16_is_the_restatement_and_monotone(api):
    vals = lg16_values()
    assert len(vals) > 90000 and vals[0] == 1 and vals[-1] > 1 << 52
    want = [ref.lg16(x) for x in vals]
    got = [api.miro_lg16(x) for x in vals]
    assert got == want
    assert ref.lg16_np(np.array(vals, np.uint64)).tolist() == want                     # the numpy form the row restatement uses
    assert all(a <= b for a, b in zip(want, want[1:]))                                 # monotone on them, sorted
    assert ref.lg16(1) == 0 and ref.lg16(2) == 1 << 16 and ref.lg16(1 << 36) == 36 << 16 and ref.lg16(3) == int(np.floor(np.log2(3.0) * 65536))
    # against floor(log2(x) * 65536) in float64: off by at most one
    off = np.array(want) - np.floor(np.log2(np.array(vals, np.float64)) * 65536.0).astype(np.int64)
    print(f"lg16 differs from floor(log2 x * 2^16) on {int((off != 0).sum())} of {len(vals)} values, by at most {int(np.abs(off).max())}")
    assert np.abs(off).max() <= 1


def test_update_is_the_restatement(api):
    tq, eq = 5 << 16, 6554
    cases_ = [(10 << 16, 5 << 16, tq, eq), (10 << 16, 0, tq, eq), (10 << 16, 52 << 16, tq, eq), (0, 1, 2, 65536), (0, 1, 3, 1), (0, 3, 1, 1),
              (ref.MU_MAX, 0, 32 << 16, 65536), (-ref.MU_MAX, 52 << 16, 1, 65536), (ref.MU_MAX - 5, 0, tq, eq), (-ref.MU_MAX + 5, 40 << 16, tq, eq),
              (7, 100, 101, 65535), (7, 100, 99, 65535), (-1 << 16, 3 << 16, tq, 1), (0, 0, 1, 32768), (0, 0, 3, 32768)]
    r = np.random.default_rng(3)
    for _ in range(20000):
        cases_.append((int(r.integers(-ref.MU_MAX, ref.MU_MAX + 1)), int(r.integers(0, (52 << 16) + 1)), int(r.integers(1, (32 << 16) + 1)),
                       int(r.integers(0, 65537))))
    for mu, s, t, e in cases_:
        assert api.miro_update(mu, s, t, e) == ref.update(mu, s, t, e), (mu, s, t, e)
    # a negative product is floored, not truncated: eta_q * (s - tau_q) = -1 -> -1 >> 16 = -1 -> mu + 1
    assert ref.update(0, 1, 2, 1) == 1 and api.miro_update(0, 1, 2, 1) == 1
    assert ref.update(0, 2, 1, 1) == 0 and api.miro_update(0, 2, 1, 1) == 0
    # both clamps
    assert api.miro_update(ref.MU_MAX, 0, 32 << 16, 65536) == ref.MU_MAX and api.miro_update(-ref.MU_MAX, 52 << 16, 1, 65536) == -ref.MU_MAX


def test_q16_and_every_range_refusal(api):
    assert api.miro_q16(5.0, 0.1) == (0, 5 << 16, 6554) == ref.q16(5.0, 0.1) and (cases.TAU_Q, cases.ETA_Q) == (5 << 16, 6554)
    assert api.miro_q16(32.0, 1.0) == (0, 32 << 16, 65536) and api.miro_q16(3.0, 0.1)[1] == 3 << 16
    for tau, eta in ((0.5, 0.25), (1e-3, 1e-3), (2.5 + 2.0 ** -17, 2.0 ** -17), (1.5 * 2.0 ** -16, 2.5 * 2.0 ** -16), (31.99999, 0.99999), (1e-9, 1e-9)):
        assert api.miro_q16(tau, eta) == ref.q16(tau, eta), (tau, eta)
    assert ref.q16(1.5 * 2.0 ** -16, 2.5 * 2.0 ** -16) == (0, 2, 2)                     # halves go to even, as lrint's default mode
    nan, inf = float("nan"), float("inf")
    for tau in (0.0, -1.0, 32.001, 33.0, nan, inf, -inf):
        assert api.miro_q16(tau, 0.1) == (ref.BAD_TAU, None, None) == ref.q16(tau, 0.1), tau
    for eta in (0.0, -0.1, 1.0001, 2.0, nan, inf, -inf):
        assert api.miro_q16(5.0, eta) == (ref.BAD_ETA, None, None) == ref.q16(5.0, eta), eta


def test_the_step_on_hand_worked_rows():
    """four equal ids: Z = 4 * 2^36, lg16(Z) = 38 bits; mu = 2 bits keeps all four exactly (L = 36 bits = lg16 of each), one unit less
    keeps the first alone; the surprise of a draw among four equal ids is 2 bits, among one 0"""
    y = np.zeros(4, np.float32)
    st = ref.Step(y, 4, 1.0, 2 << 16, 5 << 16, 6554)
    assert st.Z == 4 << 36 and st.L == 36 << 16 and st.n_keep == 4 and st.prefix
    assert st.outcome(2) == (4 << 36, 1 << 36, 2 << 16, ref.update(2 << 16, 2 << 16, 5 << 16, 6554))
    st = ref.Step(y, 4, 1.0, (2 << 16) - 1, 5 << 16, 6554)
    assert st.n_keep == 1 and st.c[0] == 0 and st.outcome(0)[:3] == (1 << 36, 1 << 36, 0)
    assert st.outcome(0)[3] == (2 << 16) - 1 + ((6554 * (5 << 16)) >> 16)
    # masses 1 : 1/2 : 1/4 : 0 (temp 1, logits in units of ln 2): -inf has no mass and is never kept, whatever mu
    y = (np.array([0.0, -1.0, -2.0, -np.inf]) * np.log(2.0)).astype(np.float32)
    for mu_bits, want in ((0, 1), (1, 1), (2, 2), (3, 3), (40, 3), (64, 3)):              # (their surprises: 0.807, 1.807, 2.807 bits)
        st = ref.Step(y, 4, 1.0, mu_bits << 16, 5 << 16, 6554)
        assert st.n_keep == want and st.prefix, (mu_bits, st.n_keep, st.L)
    assert ref.Step(y, 4, 1.0, -ref.MU_MAX, 5 << 16, 6554).n_keep == 1
    # top_k cuts first: the candidates are the first two
    assert ref.Step(y, 2, 1.0, 40 << 16, 5 << 16, 6554).n_keep == 2


def test_the_gpu_operator_tests_rows_are_a_fair_input():
    """the fairness cap, a condition and not a measurement: from the restatement alone at most 10 % of the operator test's 384 rows are
    near, at least 10 % are cut properly, and the kept set is a prefix of the candidate order on every row"""
    total = near = proper = 0
    for n_vocab in cases.VOCABS:
        x = cases.rows(n_vocab)
        ks, temps, _, _, mus = cases.requests(n_vocab)
        seen = set()
        for r in range(cases.ROWS):
            st = ref.Step(x[r], int(ks[r]), float(temps[r]), int(mus[r]), cases.TAU_Q, cases.ETA_Q)
            assert st.prefix and 1 <= st.n_lo <= st.n_keep <= st.n_hi <= st.n_cand, (n_vocab, r)
            total += 1
            near += st.near
            proper += 1 < st.n_keep < st.n_cand
            seen.add((int(ks[r]), int(mus[r])))
        assert len(seen) == len(set(ks.tolist())) * len(cases.MUS), n_vocab           # every mu meets every top_k
    print(f"near rows: {near} of {total}; rows with 1 < n_keep < n_cand: {proper}")
    assert total == 384 and near <= total // 10 and proper >= -(-total // 10)


def test_feedback_holds_the_surprise_nearer_the_target_than_a_fixed_mu():
    """400 rows of N(0, 3^2) logits at 2048 ids, temp 1, top_k = n_vocab, tau 3, eta 0.1: |mean s - tau| over the second half is smaller
    with the update than at a fixed mu = 2 tau"""
    rows = ref.chain_rows(400, 2048)
    tau_q, eta_q = ref.q16(3.0, 0.1)[1:]
    fed, near_a = ref.chain(rows, 1.0, tau_q, eta_q, True)
    fixed, near_b = ref.chain(rows, 1.0, tau_q, eta_q, False)
    a, b = ref.miss(fed, tau_q), ref.miss(fixed, tau_q)
    print(f"|mean s - tau| over the second half: {a:.4f} bits with feedback, {b:.4f} at mu = 2 tau (near steps: {near_a}, {near_b})")
    assert a < b


def test_mirostat_headers_are_exported_and_bound(api):
    names = declared_symbols("gten_hip_mirostat.h")
    assert sorted(api.MIROSTAT_SYMBOLS) == names and len(names) == 7
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "gten_hip_mirostat.h":
            assert not set(names) & set(declared_symbols(other)), other
    for name in names:
        assert hasattr(api.lib, name), name
    host = load_package().hostabi.GtenHost()
    hnames = declared_symbols("gten_host_mirostat.h")
    assert sorted(host.MIROSTAT_SYMBOLS) == hnames and len(hnames) == 9
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "gten_host_mirostat.h":
            assert not set(hnames) & set(declared_symbols(other)), other
    for name in hnames:
        assert hasattr(host.lib, name), name
    header = open(os.path.join(ROOT, "include", "gten_hip_mirostat.h")).read()
    assert "#define GTEN_HIP_MIRO_MU_MAX (64 << 16)\n" in header and api.MIRO_MU_MAX == ref.MU_MAX == 64 << 16
    assert f"#define GTEN_HIP_MIRO_INFO_BYTES {ref.INFO.itemsize}\n" in header and api.MIRO_INFO == ref.INFO and ref.INFO.itemsize == 48
    assert "#define GTEN_HIP_MIRO_MU_DEFAULT INT32_MIN" in header and api.MIRO_MU_DEFAULT == ref.MU_DEFAULT == -(1 << 31)
    # the binding lives in its own array and its own header: no older kernel header knows it
    csrc = os.path.join(ROOT, "tinyllama.cpp_amd", "csrc")
    assert "struct MiroParam" in open(os.path.join(csrc, "gten_decode_mirostat.h")).read()
    for older in ("gten_decode_sample.h", "gten_decode_nucleus.h", "gten_decode_penalty.h", "gten_decode_logprobs.h", "gten_decode_fsm.h"):
        assert "Miro" not in open(os.path.join(csrc, older)).read(), older


def test_miro_math_under_sanitizers(tmp_path):
    """lg16 at the edges and on a sweep, its monotony, the threshold's definition, the update's clamps and floor and the Q16 refusals
    (tests/host_miro_math.cpp), under ASan + UBSan.  The program includes csrc/gten_miro_math.h alone, and that header is device-free."""
    src = os.path.join(ROOT, "tests", "host_miro_math.cpp")
    includes = [line for line in open(src) if line.startswith("#include \"")]
    assert includes == ['#include "../tinyllama.cpp_amd/csrc/gten_miro_math.h"\n'], includes
    math_h = open(os.path.join(ROOT, "tinyllama.cpp_amd", "csrc", "gten_miro_math.h")).read()
    assert [line for line in math_h.split("\n") if line.startswith("#include")] == ["#include <math.h>"] and "hip/" not in math_h
    exe = str(tmp_path / "host_miro_math")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           src, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:protect_shadow_gap=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    assert "host_miro_math ok" in r.stdout


def test_cli_parses_and_refuses_mirostat():
    """every refusal comes from the option parser, before a checkpoint is opened"""
    pkg = load_package()
    pkg.build.build_all()
    cli = pkg.build.HOST_CLI

    def run(*args):
        return subprocess.run([cli, *args], capture_output=True, text=True, timeout=120)
    for args, said in ((("--mirostat", "1"), "Mirostat v1) is not implemented"), (("--mirostat", "3"), "mirostat must be 0 or 2"),
                       (("--mirostat", "-2"), "mirostat must be 0 or 2"), (("--mirostat", "x"), "Invalid mirostat value"), (("--mirostat", "2.5"), "Invalid mirostat value"),
                       (("--mirostat",), "value is missing"),
                       (("--mirostat", "2", "-greedy"), "not with -greedy"), (("-greedy", "--mirostat", "2"), "not with -greedy"),
                       (("--mirostat", "2", "--top-p", "0.9"), "do not compose"), (("--min-p", "0.1", "--mirostat", "2"), "do not compose"),
                       (("--mirostat", "2", "--score", "/nonexistent/text"), "does not apply to --score"),
                       (("--mirostat-ent", "4", "--score", "/nonexistent/text"), "does not apply to --score"),
                       (("--mirostat", "2", "--mirostat-ent", "0"), "mirostat-ent must be"), (("--mirostat-ent", "32.5"), "mirostat-ent must be"),
                       (("--mirostat-ent", "-1"), "mirostat-ent must be"), (("--mirostat-ent", "nan"), "Invalid mirostat-ent value"),
                       (("--mirostat-ent", "inf"), "Invalid mirostat-ent value"), (("--mirostat-ent", "5x"), "Invalid mirostat-ent value"),
                       (("--mirostat-lr", "0"), "mirostat-lr must be"), (("--mirostat-lr", "1.01"), "mirostat-lr must be"),
                       (("--mirostat-lr", "abc"), "Invalid mirostat-lr value"), (("--mirostat-lr",), "value is missing")):
        r = run(*args)
        assert r.returncode != 0 and said in r.stderr and "cannot open" not in r.stderr, (args, r.stderr[-300:])
    r = run("--help")
    assert r.returncode == 0 and "--mirostat N" in r.stdout and "--mirostat-ent" in r.stdout and "--mirostat-lr" in r.stdout
    # well-formed requests pass the parser, alone and beside the other stages: the next complaint is the missing checkpoint
    for args in (("--mirostat", "2"), ("--mirostat", "0"), ("--mirostat", "0", "-greedy"), ("--mirostat", "0", "--top-p", "0.9"),
                 ("--mirostat", "2", "--mirostat-ent", "32", "--mirostat-lr", "1"), ("--mirostat", "2", "--topk", "32003", "--temp", "0.8"),
                 ("--mirostat", "2", "--logprobs", "3", "--ban", "2,0", "--repeat-penalty", "1.2")):
        r = run(*args, "--model", "/nonexistent/m.gten")
        assert r.returncode != 0 and "cannot open the checkpoint" in r.stderr, (args, r.stderr[-300:])
