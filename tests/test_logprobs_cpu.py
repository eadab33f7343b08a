"""not gpu: the log-prob record's restatement (tests/logprobs_ref.py) on hand-worked rows, the new C-ABI headers
(include/gten_hip_logprobs.h, include/gten_host_logprobs.h: exported by the libraries and bound in the Python wrappers), the size of
the device's request record, and the command line's --logprobs refusals."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import logprobs_ref as ref  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402
from test_abi_loads import declared_symbols  # noqa: E402


def test_hand_worked_rows():
    # two ids at log 3 and log 1: probabilities 3/4 and 1/4
    lp, ids, lps = ref.record(np.log(np.array([1.0, 3.0])), 2, 0)
    assert ids.tolist() == [1, 0]
    assert abs(lp - np.log(0.25)) < 1e-6 and abs(lps[0] - np.log(0.75)) < 1e-6 and abs(lps[1] - lp) == 0.0
    # no chosen id: log-prob 0; n_top 0: an empty list
    lp, ids, lps = ref.record([0.0, 1.0], 0, -1)
    assert lp == 0.0 and ids.size == 0 and lps.size == 0
    # a large offset does not overflow
    assert abs(ref.lse(np.array([1000.0, 1000.0], np.float32)) - (1000.0 + np.log(2.0))) < 1e-9


def test_ties_at_the_cut_and_inside_the_list_go_to_the_lower_index():
    x = np.array([1.0, 5.0, 3.0, 3.0, 5.0, 3.0, 0.0, 3.0], np.float32)
    assert ref.order(x).tolist() == [1, 4, 2, 3, 5, 7, 0, 6]
    assert ref.record(x, 3)[1].tolist() == [1, 4, 2]                   # the cut falls inside the run of 3s: the lowest index
    assert ref.record(x, 5)[1].tolist() == [1, 4, 2, 3, 5]
    lps = ref.record(x, 5)[2]
    assert lps[0] == lps[1] and lps[2] == lps[3] == lps[4] and lps[0] > lps[2]
    assert [ref.rank(x, j) for j in (1, 4, 2, 6)] == [0, 1, 2, 7]


def test_an_all_equal_row():
    x = np.full(9, -2.5, np.float32)
    lp, ids, lps = ref.record(x, 4, 8)
    assert ids.tolist() == [0, 1, 2, 3]
    assert abs(lp + np.log(9.0)) < 1e-12 and np.allclose(lps, -np.log(9.0), atol=1e-12)


def test_more_alternatives_than_ids():
    lp, ids, lps = ref.record([0.5, 2.0, 1.0], 5, 1)
    assert ids.tolist() == [1, 2, 0, -1, -1] and lps[3:].tolist() == [0.0, 0.0] and lp == lps[0]
    lp, ids, lps = ref.record([7.0], ref.TOP, 0)
    assert ids.tolist() == [0] + [-1] * (ref.TOP - 1) and lp == 0.0 and lps[0] == 0.0


def test_signed_zeros_are_one_value():
    x = np.array([-0.0, 0.0, -1.0, 0.0, -0.0], np.float32)
    assert np.signbit(x[0]) and not np.signbit(x[1])
    assert ref.key(x)[0] == ref.key(x)[1]
    assert ref.record(x, 4)[1].tolist() == [0, 1, 3, 4]
    # and the keys order like the floats do
    v = np.array([-3e38, -1.0, -1e-40, -0.0, 1e-40, 1.0, 3e38], np.float32)
    assert (np.diff(ref.key(v)) > 0).all()


def test_logprobs_headers_are_exported_and_bound():
    pkg = load_package()
    pkg.build.build_all()
    api = pkg.hipabi.GtenHip()
    names = declared_symbols("gten_hip_logprobs.h")
    assert sorted(api.LOGPROBS_SYMBOLS) == names and len(names) == 4
    for other in ("gten_hip.h", "gten_hip_sample.h", "gten_hip_bias.h", "gten_hip_score.h"):
        assert not set(names) & set(declared_symbols(other)), other
    for name in names:
        assert hasattr(api.lib, name), name
    host = pkg.hostabi.GtenHost()
    names = declared_symbols("gten_host_logprobs.h")
    assert sorted(host.LOGPROBS_SYMBOLS) == names and len(names) == 8
    for name in names:
        assert hasattr(host.lib, name), name
    header = open(os.path.join(ROOT, "include", "gten_hip_logprobs.h")).read()
    assert f"#define GTEN_HIP_LOGPROBS_TOP {api.LOGPROBS_TOP}\n" in header and api.LOGPROBS_TOP == ref.TOP == host.LOGPROBS_TOP
    assert "#define GTEN_HIP_LOGPROBS_RECORD_BYTES 168\n" in header and 8 + 8 * ref.TOP == 168


def test_the_request_record_is_still_32_bytes():
    """the log-prob request took SampleParam's last pad word: eight 4-byte fields, and the sources assert the size at compile time"""
    csrc = os.path.join(ROOT, "tinyllama.cpp_amd", "csrc")
    text = open(os.path.join(csrc, "gten_decode_sample.h")).read()
    body = re.search(r"struct SampleParam \{(.*?)\n\};", text, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.strip().split(None, 1)[1].split(",")]
    assert len(fields) == 8 and fields[-1] == "lp1" and all(re.match(r"\s*(int|float|unsigned)\b", d) for d in body.split(";") if d.strip())
    assert "static_assert(sizeof(SampleParam) == 32" in open(os.path.join(csrc, "gten_decode_logprobs.h")).read()


@pytest.fixture(scope="module")
def cli():
    pkg = load_package()
    pkg.build.build_all()
    return pkg.build.HOST_CLI


def run(cli, *args):
    return subprocess.run([cli, *args], capture_output=True, text=True, timeout=120)


def test_cli_parses_and_refuses_logprobs(cli):
    """every refusal comes from the option parser, before a checkpoint is opened"""
    for args, said in ((("--logprobs", "21"), "logprobs must be"), (("--logprobs", "-1"), "logprobs must be"), (("--logprobs", "abc"), "Invalid logprobs value"),
                       (("--logprobs", "2x"), "Invalid logprobs value"), (("--logprobs", ""), "Invalid logprobs value"), (("--logprobs",), "value is missing")):
        r = run(cli, *args)
        assert r.returncode != 0 and said in r.stderr and "cannot open" not in r.stderr, (args, r.stderr[-300:])
    r = run(cli, "--help")
    assert r.returncode == 0 and "--logprobs" in r.stdout
    # well-formed requests pass the parser, alone and beside the constraints: the next complaint is the missing checkpoint
    for args in (("--logprobs", "0"), ("--logprobs", "20"), ("--logprobs", "5", "--ban", "2,0", "--min-new", "3"),
                 ("--logprobs", "2", "--allow", "5,6,7", "-greedy")):
        r = run(cli, *args, "--model", "/nonexistent/m.gten")
        assert r.returncode != 0 and "cannot open the checkpoint" in r.stderr, (args, r.stderr[-300:])
