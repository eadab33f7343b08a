"""not gpu: the top-p / min-p cut's restatement (tests/nucleus_ref.py) on hand-worked rows, the property that a cut never changes
an id it keeps, the new C-ABI headers (include/gten_hip_nucleus.h, include/gten_host_nucleus.h: exported by the libraries and bound in
the Python wrappers), the command line's --top-p / --min-p refusals, and the input condition of tests/test_nucleus_gpu.py's
operator test."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nucleus_cases as cases  # noqa: E402
import nucleus_ref as ref  # noqa: E402
import sample_ref as sref  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402
from test_abi_loads import declared_symbols  # noqa: E402

ONE = 1 << ref.MASS_BITS


def test_masses_three_to_one():
    """two ids with masses 3 : 1: the nucleus is the larger one alone below 3/4 and both above; at 3/4 itself the answer is the
    integer comparison q_0 >= P, and the restatement knows that this row is near"""
    y = np.log(np.array([1.0, 3.0])).astype(np.float32)
    c = ref.Cut(y, 2, 1.0, 0.76, 0.0)
    assert c.c.tolist() == [1, 0] and int(c.q[0]) == ONE and abs(int(c.q[1]) / ONE - 1 / 3) < 1e-6
    assert c.Z == int(c.q[0]) + int(c.q[1]) and c.n_nucleus == 2 and not c.near
    c = ref.Cut(y, 2, 1.0, 0.74, 0.0)
    assert c.n_nucleus == 1 and not c.near
    c = ref.Cut(y, 2, 1.0, 0.75, 0.0)
    assert c.P == int(np.floor(np.float64(c.Z) * 0.75)) and c.n_nucleus == (1 if ONE >= c.P else 2) and c.near
    # the same ratio in exact integers: four equal ids, three of them are 3/4 of the mass
    e = np.zeros(4, np.float32)
    assert ref.Cut(e, 4, 1.0, 0.75, 0.0).n_nucleus == 3 and ref.Cut(e, 4, 1.0, 0.76, 0.0).n_nucleus == 4
    assert ref.Cut(e, 4, 1.0, 0.75, 0.0).Z == 4 * ONE and ref.Cut(e, 4, 0.5, 0.5, 0.0).n_nucleus == 2


def test_a_tie_run_at_the_cut_is_an_integer_division():
    y = np.array([1.0, 3.0, 1.0, 1.0, 0.0, 1.0, 1.0], np.float32)
    c = ref.Cut(y, 7, 1.0, 0.5, 0.0)
    assert c.c.tolist() == [1, 0, 2, 3, 5, 6, 4]
    q1 = int(c.q[1])
    assert all(int(v) == q1 for v in c.q[1:6])
    for top_p in (0.3, 0.5, 0.6, 0.7, 0.8, 0.9):
        c = ref.Cut(y, 7, 1.0, top_p, 0.0)
        if ONE >= c.P:
            assert c.n_nucleus == 1
        elif c.P <= ONE + 5 * q1:
            assert c.n_nucleus == 1 + -(-(c.P - ONE) // q1), top_p        # ceil((P - mass above the run) / q) of the run, lowest indices
        else:
            assert c.n_nucleus == 7
        assert ref.order(y, 7)[: c.n_nucleus].tolist() == [1, 0, 2, 3, 5, 6, 4][: c.n_nucleus]
    # by hand: masses 1 : 5 x e^-2 : e^-3, Z = 1.7265 (in units of 2^36); 0.6 Z = 1.036 -> one of the run, 0.7 Z = 1.209 -> two,
    # 0.8 Z = 1.381 -> three, 0.9 Z = 1.554 -> all five (four reach 1.541 only)
    assert [ref.Cut(y, 7, 1.0, p, 0.0).n_nucleus for p in (0.3, 0.5, 0.6, 0.7, 0.8, 0.9)] == [1, 1, 2, 3, 4, 6]
    # top_k cuts the run first: the candidates are the lowest indices of it, and the nucleus cannot be longer
    c = ref.Cut(y, 3, 1.0, 0.99, 0.0)
    assert c.c.tolist() == [1, 0, 2] and c.n_nucleus == 3


def test_min_p_and_top_p_edges():
    y = np.array([0.5, 4.0, 3.5, -1.0, 2.0], np.float32)
    c = ref.Cut(y, 5, 1.0, 1.0, 1.0)                                   # min_p 1: t = 0, only a == 0 survives
    assert c.t == 0.0 and c.n_minp == 1 and c.n_nucleus == 5 and c.n_keep == 1
    c = ref.Cut(y, 5, 1.0, 1.0, 0.0)                                   # no cut: everything
    assert c.t == -np.inf and c.n_minp == 5 and c.n_keep == 5
    c = ref.Cut(y, 5, 1.0, 1.0, 0.5)                                   # exp(-0.5) = 0.61 >= 0.5 > exp(-2)
    assert c.n_minp == 2
    c = ref.Cut(y, 5, 2.0, 1.0, 0.5)                                   # the temperature enters: exp(-1) < 0.5 <= exp(-0.25)
    assert c.n_minp == 2 and ref.Cut(y, 5, 4.0, 1.0, 0.5).n_minp == 3
    c = ref.Cut(y, 5, 1.0, 1e-6, 0.0)                                  # top_p so small that one id remains
    assert c.n_nucleus == 1 and c.n_keep == 1
    c = ref.Cut(y, 5, 1.0, 1e-30, 0.0)                                 # P == 0: still the shortest NON-EMPTY prefix
    assert c.P == 0 and c.n_nucleus == 1
    two = np.array([4.0, 1.0, 4.0], np.float32)                        # two maxima: min_p 1 keeps both
    assert ref.Cut(two, 3, 1.0, 1.0, 1.0).n_minp == 2
    for id_, _ in (ref.draw(y, 5, 1.0, 3, s, 7, 1) for s in range(8)):
        assert id_ == 1


def test_minus_infinity_entries_have_no_mass():
    y = np.array([-np.inf, 2.0, -np.inf, 1.0], np.float32)
    c = ref.Cut(y, 4, 1.0, 0.999, 0.0)
    assert c.c.tolist() == [1, 3, 0, 2] and c.q[2:].tolist() == [0, 0] and c.Z == int(c.q[0]) + int(c.q[1])
    assert c.n_nucleus == 2 and c.n_minp == 4                          # (t = -inf: a = -inf passes the comparison, and has score -inf)
    assert ref.Cut(y, 4, 1.0, 1.0, 1e-30).n_minp == 2
    assert ref.Cut(y, 2, 1.0, 1.0, 0.0).n_cand == 2


def test_an_uncut_id_inside_the_kept_set_is_the_cut_id():
    r = np.random.default_rng(5)
    kept = changed = 0
    for i in range(300):
        n = int(r.choice([5, 64, 700]))
        y = (r.standard_normal(n) * 3.0).astype(np.float32)
        k = int(r.choice([1, 8, 40, n]))
        temp = float(r.choice([0.7, 1.0, 1.5]))
        c = ref.Cut(y, k, temp, float(r.choice([0.3, 0.9, 1.0])), float(r.choice([0.0, 0.1, 0.5])))
        plain, _ = sref.draw(y, k, temp, 11, i, 3)
        cut, _ = ref.draw(y, k, temp, 11, i, 3, c.n_keep)
        inside = plain in c.c[: c.n_keep].tolist()
        assert cut in c.c[: c.n_keep].tolist() and 1 <= c.n_keep <= c.n_cand
        if inside:
            assert cut == plain, i
            kept += 1
        else:
            changed += 1
        assert ref.draw(y, k, temp, 11, i, 3, c.n_cand)[0] == plain               # F = C: today's draw
    assert kept > 100 and changed > 20


def test_the_gpu_operator_tests_rows_are_mostly_clear_of_the_cut():
    """the input condition: the restatement's q and the device's differ by expf's error, at most delta = 2^-21 Z + 2 |C| on any sum
    (two f32 ulps per term and one count per floor); a row whose cut lies within delta of a prefix sum is `near` and only held to
    consistency on the GPU.  At least 90 % of that test's rows are not near, and every parameter value occurs among them."""
    total = near = 0
    seen = set()
    for n_vocab in cases.VOCABS:
        x = cases.rows(n_vocab)
        ks, temps, top_p, min_p, _, _ = cases.requests(n_vocab)
        for r in range(cases.ROWS):
            c = ref.Cut(x[r], ks[r], temps[r], top_p[r], min_p[r])
            assert c.delta == 2.0 ** -21 * c.Z + 2 * c.n_cand
            total += 1
            near += bool(c.near)
            if not c.near:
                seen |= {("k", int(ks[r])), ("t", float(temps[r])), ("p", float(top_p[r])), ("m", float(min_p[r]))}
    print(f"near rows: {near} of {total}")
    assert near <= total // 10
    for n_vocab in cases.VOCABS:
        assert all(("k", k) in seen for k in cases.top_ks(n_vocab))
    assert all(("t", float(np.float32(t))) in seen for t in cases.TEMPS) and all(("p", float(np.float32(p))) in seen for p in cases.TOP_PS)
    assert all(("m", float(np.float32(m))) in seen for m in cases.MIN_PS)


def test_nucleus_headers_are_exported_and_bound():
    pkg = load_package()
    pkg.build.build_all()
    api = pkg.hipabi.GtenHip()
    names = declared_symbols("gten_hip_nucleus.h")
    assert sorted(api.NUCLEUS_SYMBOLS) == names and len(names) == 3
    for other in ("gten_hip.h", "gten_hip_sample.h", "gten_hip_bias.h", "gten_hip_score.h", "gten_hip_logprobs.h"):
        assert not set(names) & set(declared_symbols(other)), other
    for name in names:
        assert hasattr(api.lib, name), name
    host = pkg.hostabi.GtenHost()
    names = declared_symbols("gten_host_nucleus.h")
    assert sorted(host.NUCLEUS_SYMBOLS) == names and len(names) == 7
    for name in names:
        assert hasattr(host.lib, name), name
    header = open(os.path.join(ROOT, "include", "gten_hip_nucleus.h")).read()
    assert f"#define GTEN_HIP_NUCLEUS_MASS_BITS {ref.MASS_BITS}\n" in header
    assert f"#define GTEN_HIP_NUCLEUS_INFO_BYTES {ref.INFO.itemsize}\n" in header and api.CUT_INFO == ref.INFO
    # the cut lives in its own array: the sampler's request record keeps its 32 bytes and its last field
    csrc = os.path.join(ROOT, "tinyllama.cpp_amd", "csrc")
    assert "struct CutParam" in open(os.path.join(csrc, "gten_decode_nucleus.h")).read()
    assert "CutParam" not in open(os.path.join(csrc, "gten_decode_sample.h")).read()


@pytest.fixture(scope="module")
def cli():
    pkg = load_package()
    pkg.build.build_all()
    return pkg.build.HOST_CLI


def run(cli, *args):
    return subprocess.run([cli, *args], capture_output=True, text=True, timeout=120)


def test_cli_parses_and_refuses_top_p_and_min_p(cli):
    """every refusal comes from the option parser, before a checkpoint is opened"""
    for args, said in ((("--top-p", "0"), "top-p must be"), (("--top-p", "1.01"), "top-p must be"), (("--top-p", "-0.5"), "top-p must be"),
                       (("--top-p", "abc"), "Invalid top-p value"), (("--top-p", "0.5x"), "Invalid top-p value"), (("--top-p", "nan"), "Invalid top-p value"),
                       (("--top-p", ""), "Invalid top-p value"), (("--top-p",), "value is missing"),
                       (("--min-p", "-0.1"), "min-p must be"), (("--min-p", "1.5"), "min-p must be"), (("--min-p", "inf"), "Invalid min-p value"),
                       (("--min-p", "x"), "Invalid min-p value"), (("--min-p",), "value is missing"),
                       (("--top-p", "0.9", "-greedy"), "not with -greedy"), (("-greedy", "--min-p", "0.1"), "not with -greedy"),
                       (("--top-p", "0.9", "--score", "/nonexistent/text"), "do not apply to --score")):
        r = run(cli, *args)
        assert r.returncode != 0 and said in r.stderr and "cannot open" not in r.stderr, (args, r.stderr[-300:])
    r = run(cli, "--help")
    assert r.returncode == 0 and "--top-p" in r.stdout and "--min-p" in r.stdout
    # well-formed requests pass the parser, alone and beside the other stages: the next complaint is the missing checkpoint
    for args in (("--top-p", "0.9"), ("--top-p", "1"), ("--min-p", "0"), ("--min-p", "1"), ("--top-p", "0.95", "--min-p", "0.05", "--topk", "32003"),
                 ("--top-p", "0.5", "--logprobs", "3", "--ban", "2,0", "--min-new", "3")):
        r = run(cli, *args, "--model", "/nonexistent/m.gten")
        assert r.returncode != 0 and "cannot open the checkpoint" in r.stderr, (args, r.stderr[-300:])
