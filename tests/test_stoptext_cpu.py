"""not gpu: stop strings given as text (include/gten_host_stoptext.h, host/stop_text_build.h).  The byte automaton is
held to the brute-force restatement of tests/stoptext_ref.py, table for table; the host expansion (the definition the device kernel is
held to) to the restatement's walk; stop_text_find to its three tie rules; every refusal to its code; a pool that mixes all four kinds of
range to the ranges built alone; and the builders run under ASan + UBSan as a stand-alone program (tests/host_text_automata.cpp)."""
import itertools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import regex_ref  # noqa: E402
import stoptext_ref as ref  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402
from test_abi_loads import declared_symbols  # noqa: E402


@pytest.fixture(scope="module")
def libs():
    pkg = load_package()
    pkg.build.build_all()
    return pkg, pkg.hipabi.GtenHip(), pkg.hostabi.GtenHost()


def test_the_headers_are_exported_and_bound(libs):
    pkg, hip, host = libs
    for header, bound, lib, n in [("gten_hip_stoptext.h", hip.STOPTEXT_SYMBOLS, hip.lib, 2), ("gten_host_stoptext.h", host.STOPTEXT_SYMBOLS, host.lib, 4),
                                  ("gten_host_json.h", host.JSON_SYMBOLS, host.lib, 1)]:
        names = declared_symbols(header)
        assert sorted(bound) == names and len(names) == n, header
        for name in names:
            assert hasattr(lib, name), name


SETS = [
    [b"a"],                                             # one 1-byte string
    [b"abcab", b"ab"],                                  # a string and its own suffix
    [b"aba", b"bab"],                                   # overlapping strings
    [b"\nUser:", b"</answer>", b"</a"],
    [b"\xff\x80", b"\x80\xff\x80", b"\x00", b"a\x00b"],  # bytes >= 0x80 and 0x00
    [b"aaaa", b"aa", b"a"],
    ["été".encode(), "é".encode()],
]


@pytest.mark.parametrize("strings", SETS, ids=[str(k) for k in range(len(SETS))])
def test_the_automaton_equals_the_brute_force_restatement(libs, strings):
    pkg, _, host = libs
    want, want_acc = ref.dfa(strings)
    got, acc = host.stop_text_dfa(strings)
    assert got.shape == want.shape and (got == want).all() and (acc == want_acc).all()
    assert int(got.max()) < len(acc)                                     # total: no entry is "no edge"
    # canonical: any order, any repetition
    for perm in itertools.islice(itertools.permutations(strings), 6):
        again, again_acc = host.stop_text_dfa(list(perm) + [perm[0]])
        assert again.tobytes() == got.tobytes() and again_acc.tobytes() == acc.tobytes()


def test_the_automaton_accepts_exactly_where_a_string_has_just_ended(libs):
    pkg, _, host = libs
    g = np.random.default_rng(5)
    strings = [b"abcab", b"ab", b"bca", b"cc"]
    n256, acc = host.stop_text_dfa(strings)
    text = bytes(g.choice(list(b"abc"), 400).tolist())
    s = 0
    for k, c in enumerate(text):
        s = int(n256[s][c])
        assert bool(acc[s]) == any(text[:k + 1].endswith(x) for x in strings), k


# empty pieces (0, 5, 13), 1-byte pieces, a piece that holds the whole string with bytes behind it (8), one that ends exactly on it (9),
# a pair the string straddles (10 + 11), pieces with bytes >= 0x80
PIECES = [b"", b"a", b"b", b"c", b"</", b"", b"answer>", b"x", b"<</answer>yy", b"..</answer>", b"abc</ans", b"wer>abc", b"\xc3\xa9", b"",
          b"</answer", b">", b"ab", b"cab", b"abcab", b"bcabc"]


def test_the_host_expansion_equals_the_restatement(libs):
    pkg, hip, host = libs
    V = len(PIECES)
    f = pkg.hostabi.Fsm(host, V)
    f.set_vocab(PIECES)
    front = np.tile(np.arange(2, dtype=np.uint16)[:, None], (1, V))
    assert f.add_table(front, np.zeros(2, np.uint8)) == 0                # every range below has base > 0
    ranges = []
    for strings in ([b"</answer>"], [b"abcab", b"ab"], [b"\xa9", b"c"]):
        base = f.add_stop_text(strings)
        ranges.append((base, strings))
    nxt, flags = f.tables()
    assert f.n_search == 3 and f.n_regex == 0
    for base, strings in ranges:
        n256, acc = ref.dfa(strings)
        rows, fl = ref.expand(n256, acc, PIECES, base)
        Sb = len(acc)
        assert (nxt[base:base + Sb + 1] == rows).all() and (flags[base:base + Sb + 1] == fl).all(), strings
        # nothing is banned below the HIT state; an empty piece stays where it is
        assert (rows[:Sb] != ref.DEAD).all() and all((rows[:Sb, i] == base + np.arange(Sb)).all() for i in (0, 5, 13))
    base = ranges[0][0]
    hit = base + len(ref.dfa([b"</answer>"])[1])
    assert nxt[base][8] == hit and nxt[base][9] == hit                    # the whole string inside a piece, with and without a tail
    mid = nxt[base][10]
    assert mid not in (hit, base) and nxt[mid][11] == hit                 # the straddling pair: the second piece completes it
    assert nxt[base][11] != hit and nxt[nxt[base][4]][6] == hit          # "wer>abc" alone does not; "</" + "answer>" does
    assert hip.fsm_check(nxt, flags, V) == (0, -1)
    f.close()


def test_find_reports_the_first_end_then_the_longest_then_the_lowest_index(libs):
    pkg, _, host = libs
    cases = [
        ([b"yy", b"b"], b"aabyy"),                      # "b" ends first although "yy" is listed first
        ([b"b", b"ab", b"aab"], b"xaab"),               # three end at the same byte: the longest
        ([b"ab", b"b", b"ab"], b"ab"),                  # equal strings: the lowest index
        ([b"abc", b"bc", b"c"], b"zzabc"),
        ([b"q"], b"no match here"),
        ([b"a"], b""),
        ([b"\x00\xff"], b"a\x00\xffb"),
        ([b"long string"], b"long strin"),
    ]
    want = [(1, 2, 3), (2, 1, 4), (0, 0, 2), (0, 2, 5), (-1, 13, 13), (-1, 0, 0), (0, 1, 3), (-1, 10, 10)]
    for (strings, text), w in zip(cases, want):
        assert ref.find(strings, text) == w, (strings, text)
        assert host.stop_text_find(strings, text) == w, (strings, text)
    g = np.random.default_rng(11)
    for _ in range(200):
        strings = [bytes(g.choice(list(b"ab"), int(g.integers(1, 4))).tolist()) for _ in range(int(g.integers(1, 4)))]
        text = bytes(g.choice(list(b"abc"), int(g.integers(0, 12))).tolist())
        assert host.stop_text_find(strings, text) == ref.find(strings, text), (strings, text)


def test_refusals(libs):
    pkg, _, host = libs
    for bad in ([], [b""], [b"a", b""]):
        with pytest.raises(ValueError, match="-1"):
            host.stop_text_dfa(bad)
    with pytest.raises(ValueError, match="-2"):                         # 65534 nodes with the root: one more than fits
        host.stop_text_dfa([b"a" * 32767, b"b" * 32766])
    assert len(host.stop_text_dfa([b"a" * 32766, b"b" * 32766])[1]) == 65533
    with pytest.raises(ValueError):
        host.stop_text_find([b""], b"abc")
    f = pkg.hostabi.Fsm(host, 4)
    with pytest.raises(ValueError, match="-1"):                         # no vocabulary yet
        f.add_stop_text([b"a"])
    f.set_vocab([b"", b"a", b"b", b"ab"])
    for bad in ([], [b""]):
        with pytest.raises(ValueError, match="-1"):
            f.add_stop_text(bad)
    assert f.n_states == 0                                              # a refusal leaves the pool as it was
    assert f.add_stop_text([b"ab"]) == 0 and f.n_states == 4
    with pytest.raises(ValueError):                                     # the vocabulary is fixed once a search range exists
        f.set_vocab([b"", b"a", b"b", b"ab"])
    f.close()
    big = pkg.hostabi.Fsm(host, 40000)                                  # the pool's own limits: 2^30 bytes of table
    big.set_vocab([b"a"] * 40000)
    with pytest.raises(ValueError, match="-2"):
        big.add_stop_text([b"a" * 14000])
    assert big.n_states == 0
    big.close()


def test_a_pool_that_mixes_every_kind_of_range_relocates_each(libs):
    pkg, hip, host = libs
    pieces = regex_ref.synthetic_vocab(300, 21, b'ab01 .\n{}":,truefals')
    V = len(pieces)
    schema = {"type": "object", "properties": {"a": {"type": "boolean"}}, "required": ["a"]}
    pattern = host.json_schema_regex(schema)

    def alone(add):
        f = pkg.hostabi.Fsm(host, V)
        f.set_vocab(pieces)
        assert add(f) == 0
        out = f.tables()
        f.close()
        return out

    adds = [lambda f: f.add_stop([[5, 6], [7]]), lambda f: f.add_regex("[ab]+ [01]", 0), lambda f: f.add_stop_text([b"ab", b"0."]),
            lambda f: f.add_json_schema(schema, 0), lambda f: f.add_stop_text([b"\n"]), lambda f: f.add_choices([[9, 10], [3]])]
    f = pkg.hostabi.Fsm(host, V)
    f.set_vocab(pieces)
    bases = [add(f) for add in adds]
    nxt, flags = f.tables()
    assert f.n_search == 2 and f.n_regex == 2 and bases == sorted(bases) and bases[0] == 0
    assert f.add_regex(pattern, 0) == bases[3]                           # add_json_schema is add_regex of the schema's pattern
    for add, base in zip(adds, bases):
        rows, fl = alone(add)
        moved = np.where(rows == ref.DEAD, rows, rows + base).astype(np.uint16)
        assert (nxt[base:base + len(fl)] == moved).all() and (flags[base:base + len(fl)] == fl).all(), base
    assert bases[-1] + len(alone(adds[-1])[1]) == f.n_states
    assert hip.fsm_check(nxt, flags, V) == (0, -1)
    f.close()


def test_builders_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/host_text_automata.cpp: a stand-alone program (its own main, nothing loaded into Python) over host/stop_text_build.h,
    host/json_schema.h and host/regex_build.h, fed the inputs of these tests plus malformed and truncated schemas"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "host_text_automata")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tinyllama.cpp_amd"), os.path.join(ROOT, "tests", "host_text_automata.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:protect_shadow_gap=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    assert "host_text_automata ok" in r.stdout


def test_the_command_line_refuses_what_it_cannot_bind(libs, tmp_path):
    """--stop-text and --json-schema are refused beside the other automaton flags, with the flag's name in the message, before any file
    of the model is opened"""
    pkg, _, _ = libs
    cli = pkg.build.HOST_CLI
    good = tmp_path / "schema.json"
    good.write_text('{"type": "boolean"}')
    bad = tmp_path / "bad.json"
    bad.write_text('{"type": "integer", "minimum": 3}')
    broken = tmp_path / "broken.json"
    broken.write_text('{"type": ')
    for args, what in [(["--stop-text", "a", "--stop", "5"], "--stop-text and --stop"), (["--choice", "5", "--stop-text", "a"], "--stop-text and --choice"),
                       (["--stop-text", "a", "--regex", "b"], "--stop-text and --regex"), (["--stop-text"], "stop-text value is missing"),
                       (["--stop-text", ""], "--stop-text: an empty string"),
                       (["--json-schema", str(good), "--regex", "b"], "--json-schema and --regex"), (["--json-schema", str(good), "--stop", "5"], "--json-schema and --stop"),
                       (["--json-schema", str(good), "--choice", "5"], "--json-schema and --choice"),
                       (["--json-schema", str(good), "--stop-text", "a"], "--json-schema and --stop-text"),
                       (["--json-schema"], "json-schema value is missing"), (["--json-schema", str(tmp_path / "none.json")], "--json-schema: cannot read"),
                       (["--json-schema", str(bad)], "--json-schema: unsupported: /minimum"), (["--json-schema", str(broken)], "--json-schema: malformed JSON at byte 9")]:
        r = subprocess.run([cli, *args], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and what in r.stderr, (args, r.stderr[-400:])
    for args in (["--stop-text", "abc", "--stop-text", "\\n"], ["--json-schema", str(good)]):
        r = subprocess.run([cli, *args, "--model", "/nonexistent/x.gten", "-p", "hi"], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "cannot open the checkpoint" in r.stderr, (args, r.stderr[-400:])      # good values get as far as the files
    usage = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--stop-text STRING" in usage and "--json-schema FILE" in usage
