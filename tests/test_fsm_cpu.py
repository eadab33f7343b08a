"""not gpu: the token automata's builders (host/fsm_build.h through gten_host_fsm_*) against the brute-force restatement
(tests/fsm_ref.py), the upload validation that needs no device (gten_hip_fsm_check), the new C-ABI headers (include/gten_hip_fsm.h,
include/gten_host_fsm.h: exported by the libraries and bound in the Python wrappers), the host's fsm_ok, and the command line's
refusals."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fsm_ref as ref  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402
from test_abi_loads import declared_symbols  # noqa: E402


@pytest.fixture(scope="module")
def libs():
    pkg = load_package()
    pkg.build.build_all()
    return pkg, pkg.hipabi.GtenHip(), pkg.hostabi.GtenHost()


def test_the_restatement_by_hand():
    """tests/fsm_ref.py alone, against cases worked out by hand: it runs none of the project's code (so it passes on any commit); the
    other tests hold the project to this restatement"""
    # states: 0 -a-> 1 -b-> 2 (final); everything else back to 0; over ids {0: a, 1: b, 2: c}
    nxt = np.array([[1, 0, 0], [1, 2, 0], [0, 0, 0]], np.uint16)
    flags = np.array([0, 0, 1], np.uint8)
    assert ref.walk(nxt, flags, 0, [2, 0, 0, 1, 2, 0]) == [0, 1, 1, 2, 2, 2]                # carried on once final
    assert ref.first_final(nxt, flags, 0, [2, 0, 0, 1, 2]) == 3 and ref.first_final(nxt, flags, 0, [0, 2, 1]) is None
    assert ref.stop_scan([2, 0, 0, 1, 2], [[0, 1]]) == 3 and ref.stop_scan([0, 2, 1], [[0, 1]]) is None
    assert ref.stop_scan([5, 5, 7], [[7], [5, 5]]) == 1 and ref.stop_scan([], [[1]]) is None
    banned = np.array([[ref.DEAD, 1, ref.DEAD], [0, 0, 0]], np.uint16)
    x = np.array([1.5, -0.0, 0.0], np.float32)
    y = ref.mask_row(x, banned, np.array([0, 1], np.uint8), 0)
    assert y[0] == -np.inf and y[2] == -np.inf and y.view(np.uint32)[1] == x.view(np.uint32)[1]      # the signed zero keeps its bits
    assert (ref.mask_row(x, banned, np.array([0, 1], np.uint8), 1).view(np.uint32) == x.view(np.uint32)).all()   # final: not masked
    assert (ref.mask_row(x, banned, np.array([0, 1], np.uint8), -1).view(np.uint32) == x.view(np.uint32)).all()
    assert ref.walk(banned, np.array([0, 1], np.uint8), 0, [0, 1]) == [ref.DEAD, ref.DEAD]


STOP_LISTS = {
    2: [[[0, 1]], [[0, 0, 1], [0, 1]], [[1, 1, 0], [1, 0], [0]], [[0, 1, 0, 1], [1, 0, 1], [1, 1]], [[1], [0, 0, 0, 0, 0]]],
    5: [[[3]], [[0, 1, 2], [1, 2]], [[4, 4], [4, 3, 4], [2, 4, 3]], [[0, 1, 2, 3, 4], [2, 3], [3, 4, 0]], [[1, 1, 1], [1, 1], [2, 1, 1, 1]]],
}


@pytest.mark.parametrize("alphabet", [2, 5])
def test_add_stop_is_final_exactly_at_the_scans_position(libs, alphabet):
    pkg, _, host = libs
    g = np.random.default_rng(11 + alphabet)
    hits = 0
    for stops in STOP_LISTS[alphabet]:                        # (overlaps, and lists in which one sequence is a suffix of another)
        f = pkg.hostabi.Fsm(host, alphabet)
        start = f.add_stop(stops)
        nxt, flags = f.tables()
        assert start == 0 and (nxt != ref.DEAD).all() and (nxt < f.n_states).all(), "a stop automaton bans nothing"
        assert ref.check(nxt, flags, len(flags), alphabet) == ref.OK
        for trial in range(200):
            ids = g.integers(0, alphabet, int(g.integers(0, 24))).tolist()
            want = ref.stop_scan(ids, stops)
            assert ref.first_final(nxt, flags, start, ids) == want, (stops, ids)
            hits += want is not None
        f.close()
    assert hits > 100


def test_add_choices_allows_exactly_the_tries_edges(libs):
    pkg, _, host = libs
    V = 7
    choices = [[1, 2, 3], [1, 2, 4], [5], [6, 6, 6, 0], [1, 3]]
    f = pkg.hostabi.Fsm(host, V)
    start = f.add_choices(choices)
    nxt, flags = f.tables()
    edges, whole = ref.trie_edges(choices)
    seen = set()
    def visit(state, prefix):
        seen.add(state)
        if prefix in whole:
            assert flags[state] & ref.FINAL and (nxt[state] == ref.DEAD).all(), prefix
            return
        assert not flags[state] & ref.FINAL
        allowed = {i for i in range(V) if nxt[state][i] != ref.DEAD}
        assert allowed == edges[prefix], (prefix, allowed)
        for i in allowed:
            visit(int(nxt[state][i]), prefix + (i,))
    visit(start, ())
    assert len(seen) == f.n_states == 1 + sum(len(v) for v in edges.values())
    for c in choices:
        assert ref.first_final(nxt, flags, start, c) == len(c) - 1
    # the prefix case, both orders, an equal pair and an empty choice are refused; the pool is as it was
    for bad in ([[1, 2], [1, 2, 3]], [[1, 2, 3], [1, 2]], [[4], [4]], [[1], []]):
        with pytest.raises(ValueError):
            f.add_choices(bad)
        assert f.n_states == len(flags)
    with pytest.raises(ValueError):
        f.add_choices([[1, V]])                               # an id outside the vocabulary
    with pytest.raises(ValueError):
        f.add_stop([[1], []])                                 # an empty stop sequence
    with pytest.raises(ValueError):
        f.add_stop([[-1]])
    assert f.n_states == len(flags)
    f.close()


def test_add_table_relocates_and_automata_do_not_see_each_other(libs):
    pkg, _, host = libs
    V = 5
    g = np.random.default_rng(5)
    f = pkg.hostabi.Fsm(host, V)
    stops = [[0, 1], [3]]
    a = f.add_stop(stops)
    n_a = f.n_states
    own, own_flags = ref.random_pool(g, 6, V, density=0.5, n_final=2)
    b = f.add_table(own, own_flags)
    n_b = f.n_states
    choices = [[2, 2], [4]]
    c = f.add_choices(choices)
    nxt, flags = f.tables()
    assert (a, b, c) == (0, n_a, n_b) and f.n_states == n_b + 4 and nxt.shape == (f.n_states, V)
    # the caller's table, shifted by its base, DEAD left alone
    want = own.astype(np.int64) + b
    want[own == ref.DEAD] = ref.DEAD
    assert (nxt[b:n_b] == want).all() and (flags[b:n_b] == own_flags).all()
    # every automaton stays inside its own range of states
    for lo, hi in ((a, n_a), (b, n_b), (c, f.n_states)):
        live = nxt[lo:hi][nxt[lo:hi] != ref.DEAD]
        assert ((live >= lo) & (live < hi)).all()
    # ... and each still does what it did alone
    for trial in range(100):
        ids = g.integers(0, V, 12).tolist()
        assert ref.first_final(nxt, flags, a, ids) == ref.stop_scan(ids, stops)
        assert [s - b if s != ref.DEAD else s for s in ref.walk(nxt, flags, b, ids)] == ref.walk(own, own_flags, 0, ids)
    assert ref.first_final(nxt, flags, c, [2, 2]) == 1 and ref.first_final(nxt, flags, c, [4]) == 0
    assert ref.check(nxt, flags, len(flags), V) == ref.OK
    # entries that are neither a state of the table nor DEAD are refused
    bad = own.copy()
    bad[bad != ref.DEAD] = 6
    with pytest.raises(ValueError):
        f.add_table(bad, own_flags)
    assert f.n_states == len(flags)
    f.close()
    # the pool's size limit: 65535 states in all
    f = pkg.hostabi.Fsm(host, 2)
    big = np.zeros((40000, 2), np.uint16)
    assert f.add_table(big, np.zeros(40000, np.uint8)) == 0
    with pytest.raises(ValueError):
        f.add_table(big, np.zeros(40000, np.uint8))
    assert f.add_table(big[:25535], np.zeros(25535, np.uint8)) == 40000 and f.n_states == 65535
    f.close()
    with pytest.raises(ValueError):
        pkg.hostabi.Fsm(host, 0)


def test_upload_validation_without_a_device(libs):
    _, api, _ = libs
    V = 3
    good = np.array([[1, ref.DEAD, 0], [ref.DEAD, ref.DEAD, ref.DEAD]], np.uint16)
    flags = np.array([0, 1], np.uint8)
    assert api.fsm_check(good, flags, V) == (ref.OK, -1) == (ref.check(good, flags, 2, V), -1)
    # S outside [1, 65535]
    assert api.fsm_check(good, flags, V, n_states=0)[0] == ref.BAD_STATES == ref.check(good, flags, 0, V)
    assert api.fsm_check(good, flags, V, n_states=65536)[0] == ref.BAD_STATES == ref.check(good, flags, 65536, V)
    assert api.fsm_check(good, flags, V, n_states=-1)[0] == ref.BAD_STATES
    # S * n_vocab * 2 above GTEN_HIP_FSM_MAX_BYTES (decided before a table is read): 16385 states of 32768 ids are 2^30 + 65536 bytes
    assert api.fsm_check(good, flags, 32768, n_states=16385)[0] == ref.TOO_LARGE == ref.check(good, flags, 16385, 32768)
    assert api.fsm_check(good, flags, 65535, n_states=8193)[0] == ref.TOO_LARGE
    assert 16384 * 32768 * 2 == ref.MAX_BYTES == api.FSM_MAX_BYTES          # (exactly the limit is allowed: the GPU tests upload no such pool)
    # an entry that is neither below S nor DEAD
    bad = good.copy()
    bad[1, 2] = 2
    assert api.fsm_check(bad, flags, V) == (ref.BAD_ENTRY, 1) and ref.check(bad, flags, 2, V) == ref.BAD_ENTRY
    bad[1, 2] = 0xFFFE
    assert api.fsm_check(bad, flags, V)[0] == ref.BAD_ENTRY
    # a non-final state without an allowed id; a final one may have none
    assert api.fsm_check(good, np.array([0, 0], np.uint8), V) == (ref.STUCK, 1) and ref.check(good, np.array([0, 0], np.uint8), 2, V) == ref.STUCK
    stuck0 = np.full((1, V), ref.DEAD, np.uint16)
    assert api.fsm_check(stuck0, np.array([0], np.uint8), V) == (ref.STUCK, 0)
    assert api.fsm_check(stuck0, np.array([1], np.uint8), V)[0] == ref.OK
    # the largest pool of states: state 65534 exists, 65535 is DEAD
    big = np.full((65535, 2), 65534, np.uint16)
    assert api.fsm_check(big, np.zeros(65535, np.uint8), 2)[0] == ref.OK


def test_fsm_headers_are_exported_and_bound(libs):
    pkg, api, host = libs
    names = declared_symbols("gten_hip_fsm.h")
    assert sorted(api.FSM_SYMBOLS) == names and len(names) == 7
    others = ("gten_hip.h", "gten_hip_sample.h", "gten_hip_bias.h", "gten_hip_score.h", "gten_hip_logprobs.h", "gten_hip_nucleus.h", "gten_hip_penalty.h",
              "gten_hip_prefix.h", "gten_hip_prefix_decode.h", "gten_hip_ab.h")
    for other in others:
        assert not set(names) & set(declared_symbols(other)), other
    for name in names:
        assert hasattr(api.lib, name), name
    hnames = declared_symbols("gten_host_fsm.h")
    assert sorted(host.FSM_SYMBOLS) == hnames and len(hnames) == 19
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other.startswith("gten_host") and other != "gten_host_fsm.h":
            assert not set(hnames) & set(declared_symbols(other)), other
    for name in hnames:
        assert hasattr(host.lib, name), name
    header = open(os.path.join(ROOT, "include", "gten_hip_fsm.h")).read()
    assert "#define GTEN_HIP_FSM_DEAD 0xFFFF\n" in header and api.FSM_DEAD == ref.DEAD == 0xFFFF
    assert "#define GTEN_HIP_FSM_MAX_BYTES (1ull << 30)" in header and "#define GTEN_HIP_FSM_MAX_STATES 65535\n" in header
    # the binding lives in its own array: no older kernel header knows it
    csrc = os.path.join(ROOT, "tinyllama.cpp_amd", "csrc")
    assert "struct FsmParam" in open(os.path.join(csrc, "gten_decode_fsm.h")).read()
    for older in ("gten_decode_sample.h", "gten_decode_nucleus.h", "gten_decode_penalty.h", "gten_decode_logprobs.h"):
        assert "FsmParam" not in open(os.path.join(csrc, older)).read(), older


FSM_OK_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "host/generate.h"
int main(int argc, char** argv)
{
    for (int i = 1; i + 1 < argc; i += 2) std::printf("%d\n", gten::fsm_ok(std::atoi(argv[i]), std::atoi(argv[i + 1])) ? 1 : 0);
    gten::Request r;
    gten::Requests rs;
    const int32_t starts[2] = {-1, 7};
    std::printf("%d %d %d %d\n", r.fsm_start, rs[0].fsm_start, rs.bound_to(starts)[1].fsm_start, (int)gten::kFsm);
    const int32_t tables[2] = {-1, 3};
    rs.table = {tables, -1};
    std::printf("%d %d\n", rs.bound_to(starts).ok(1, 0) ? 1 : 0, rs.bound_to(starts).ok(2, 0) ? 1 : 0);
    return 0;
}
"""


def test_host_fsm_ok_and_request_defaults(tmp_path):
    """host/generate.h's checks, compiled alone (the header names the device library only inside templates nobody instantiates here)"""
    src, exe = tmp_path / "fsm_ok.cpp", tmp_path / "fsm_ok"
    src.write_text(FSM_OK_MAIN)
    pkg_dir = os.path.join(ROOT, "tinyllama.cpp_amd")
    r = subprocess.run(["g++", "-std=c++17", "-O0", "-fopenmp", "-I" + os.path.join(ROOT, "include"), "-I" + pkg_dir, "-o", str(exe), str(src),
                        "-L" + os.path.join(pkg_dir, "csrc"), "-lgten_hip", "-Wl,-rpath," + os.path.join(pkg_dir, "csrc")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = [((-1, -1), 1), ((0, -1), 1), ((65534, -1), 1), ((65535, -1), 0), ((-2, -1), 0), ((-1, 3), 1), ((0, 0), 0), ((5, 15), 0)]
    out = subprocess.run([str(exe), *[str(v) for c, _ in cases for v in c]], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split("\n")
    assert [int(v) for v in lines[: len(cases)]] == [w for _, w in cases]
    assert lines[len(cases)] == "-1 -1 7 32"                  # Request::fsm_start defaults to -1; stage bit kFsm = 32
    assert lines[len(cases) + 1] == "1 0"                     # a table and an automaton on one item are refused


def run(cli, *args):
    return subprocess.run([cli, *args], capture_output=True, text=True, timeout=120)


def test_cli_parses_and_refuses_the_automaton_flags(libs):
    """every refusal comes from the option parser, before a checkpoint is opened"""
    cli = libs[0].build.HOST_CLI
    for args, said in ((("--stop", ""), "Invalid stop value"), (("--stop", "1,x"), "Invalid stop value"), (("--stop", "1,,2"), "Invalid stop value"),
                       (("--stop", "40000"), "stop ids must be"), (("--stop", "-1"), "stop ids must be"), (("--stop",), "value is missing"),
                       (("--choice", "a"), "Invalid choice value"), (("--choice", "32003"), "choice ids must be"), (("--choice",), "value is missing"),
                       (("--stop", "1,2", "--choice", "3"), "do not combine"), (("--stop", "1", "--ban", "2"), "do not combine with --ban"),
                       (("--choice", "1", "--allow", "2,3"), "do not combine with --ban"), (("--choice", "1,2", "--choice", "1,2,3"), "prefix of another"),
                       (("--choice", "1,2", "--choice", "1,2"), "prefix of another"), (("--stop", "1", "--score", "/nonexistent/text"), "do not apply to --score")):
        r = run(cli, *args)
        assert r.returncode != 0 and said in r.stderr and "cannot open" not in r.stderr, (args, r.stderr[-300:])
    r = run(cli, "--help")
    assert r.returncode == 0 and "--stop" in r.stdout and "--choice" in r.stdout
    # well-formed requests pass the parser, with -greedy too, repeated, with a repeated id, beside the other stages
    for args in (("--stop", "13"), ("--stop", "5,5,7", "--stop", "7"), ("-greedy", "--stop", "2"), ("--choice", "9,8", "--choice", "9,7", "--choice", "3"),
                 ("-greedy", "--choice", "1,1"), ("--stop", "2", "--top-p", "0.9", "--repeat-penalty", "1.1", "--logprobs", "2")):
        r = run(cli, *args, "--model", "/nonexistent/m.gten")
        assert r.returncode != 0 and "cannot open the checkpoint" in r.stderr, (args, r.stderr[-300:])
