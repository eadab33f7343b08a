"""not gpu: regular expressions as token automata (include/gten_host_regex.h, host/regex_build.h).  The compiler is held
to Python's re (a byte string is accepted iff it is valid UTF-8 and re.fullmatch(pattern, text, re.ASCII) matches), its refusals to
their codes and offsets, its output to the canonical form; the host expansion over the vendored vocabulary to the walk of
tests/regex_ref.py; and the whole of it runs under ASan + UBSan as a stand-alone program (tests/host_sanitize_regex.cpp)."""
import itertools
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

import regex_ref as ref  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402
from test_abi_loads import declared_symbols  # noqa: E402

VOCAB = os.path.join(ROOT, "tests", "golden", "tokenizer.bin")
N_VOCAB = 32003


@pytest.fixture(scope="module")
def libs():
    pkg = load_package()
    pkg.build.build_all()
    return pkg, pkg.hipabi.GtenHip(), pkg.hostabi.GtenHost()


@pytest.fixture(scope="module")
def vocab(libs):
    pkg, _, host = libs
    t = host.tokenizer(VOCAB)
    v = t.vocab_bytes(N_VOCAB)
    t.close()
    return v


def test_the_headers_are_exported_and_bound(libs):
    pkg, hip, host = libs
    names = declared_symbols("gten_hip_regex.h")
    assert sorted(hip.REGEX_SYMBOLS) == names and len(names) == 4
    for n in names:
        assert hasattr(hip.lib, n), n
    names = declared_symbols("gten_host_regex.h")
    assert sorted(host.REGEX_SYMBOLS) == names and len(names) == 5
    for n in names:
        assert hasattr(host.lib, n), n


# every construct of the dialect: nested groups, the {m,n} edges, classes with - and ] escaped, `.` beside multi-byte literals,
# alternations with common prefixes, patterns that accept the empty string
PATTERNS = [
    "a", "ab", "a|b", "[ab]", "aa*", "a+", "(ab)?", "(?:ab|)", "a{0}", "a{0,1}", "a{3,}", "a{2}", "a{1,3}b", "(ab){2}", "(a|b){0,2}",
    r"[a\-\]]+", r"[\]a-]b", "[a-c]x", "[^a]", "[^ab]b", r"[^\n]a", r"[\d_]+", r"[^\w]", r"[\D]", r"[\s.]a",
    ".", "..", ".*", ".é", "é.", "é+", "(é|a)*", "😀?a", ".😀",
    r"\d", r"\d+\.\d*", r"\D", r"\w\W", r"\s*\S", r"\w+@\w+",
    r"\n", r"\t|\r|\f|\v", r"\x41\x0a", r"\.\*\+\?\(\)\[\]\{\}\|\\\^\$", r"a\ b",
    "abc|abd|ab", "(a|ab)(c|bcd)", "a(b|c(d|e)*f)*g", "((a))", "(a(b(c)?)*)+", "(?:a|(?:b|c))d", "(|a)b", "a||b", "x*y*", "(a*)*", "(a?){3}",
    r'\{"k": [0-9]{1,3}\}', "}a", "a]", ".*a.", "(a|b)*abb",
]


def alphabet_of(pattern):
    """up to four characters of the pattern itself, then a digit, \\n, a two-byte and a four-byte code point"""
    own = []
    for kind in (str.isalpha, str.isdigit, lambda c: c in ' .@_-]}{":'):                 # letters first, then digits, then punctuation
        for c in pattern:
            if kind(c) and c not in own and ord(c) < 128:
                own.append(c)
    return own[:4] + ["7", "\n", "é", "😀"]


BROKEN = [b"\xc3", b"\xf0\x9f\x98", b"\xc0\x80", b"\xe0\x80\x80", b"\xed\xa0\x80", b"\xff", b"\x80", b"\xf4\x90\x80\x80", b"\xf8\x88\x80\x80\x80",
          b"\xc3\x28", b"\xe2\x82", b"\xf0\x80\x80\x80"]


def test_the_compiler_agrees_with_re_on_every_short_string(libs):
    pkg, _, host = libs
    assert len(PATTERNS) >= 40
    empties, unmatched = 0, []
    for p in PATTERNS:
        n256, acc = pkg.hostabi.byte_dfa(host, p)
        rx = re.compile(p, re.ASCII)
        empties += bool(acc[0])
        chars = alphabet_of(p)
        some = 0
        for L in range(5):
            for t in itertools.product(chars, repeat=L):
                s = "".join(t)
                want = rx.fullmatch(s) is not None
                some += want
                assert ref.accepts(n256, acc, s.encode()) == want, (p, s)
        unmatched += [p] if not some else []
        # truncated, overlong, surrogate and out-of-range byte strings are never accepted, alone or around accepted text
        for b in BROKEN:
            for pre, post in ((b"", b""), (b"a", b""), (b"", b"a"), ("é".encode(), b""), (b"", "😀".encode())):
                assert not ref.accepts(n256, acc, pre + b + post), (p, pre + b + post)
    assert empties >= 8
    # (patterns none of whose short strings match get strings of their own below)
    assert set(unmatched) <= {r"\x41\x0a", r"\.\*\+\?\(\)\[\]\{\}\|\\\^\$", r"\t|\r|\f|\v", r'\{"k": [0-9]{1,3}\}', "a(b|c(d|e)*f)*g"}, unmatched
    # the long literal ones, on strings of their own
    for p, yes, no in [(r"\x41\x0a", "A\n", "A"), (r"\.\*\+\?\(\)\[\]\{\}\|\\\^\$", ".*+?()[]{}|\\^$", ".*"), (r'\{"k": [0-9]{1,3}\}', '{"k": 042}', '{"k": 0421}'),
                       (r"\w+@\w+", "a_1@b", "a@"), ("a(b|c(d|e)*f)*g", "acdedfbg", "acdg"), ("(a|b)*abb", "babb", "bab")]:
        n256, acc = pkg.hostabi.byte_dfa(host, p)
        assert ref.accepts(n256, acc, yes.encode()) and re.fullmatch(p, yes, re.ASCII)
        assert not ref.accepts(n256, acc, no.encode()) and not re.fullmatch(p, no, re.ASCII)


# (pattern, code, byte offset of the offence)
REFUSED = [
    ("", -1, 0), ("()", -1, 0), ("(?:)", -1, 0), ("(a", -1, 0), ("a)", -1, 1), ("ab(c|d", -1, 2), ("[", -1, 0), ("[]", -1, 1), ("[^]", -1, 2), ("[a", -1, 0), ("[z-a]", -1, 1),
    (r"[a-\d]", -1, 1), (r"[\d-z]", -1, 1), ("*a", -1, 0), ("a|*", -1, 2), ("a**", -1, 2), ("a{2}{3}", -1, 4), ("a+*", -1, 2), ("a{", -1, 1), ("a{x}", -1, 1), ("a{,3}", -1, 1),
    ("a{2,1}", -1, 1), ("{2}", -1, 0), ("a\\", -1, 1), (r"\q", -1, 0), (r"\xg0", -1, 0), (r"\x4", -1, 0),
    ("^a", -4, 0), ("a$", -4, 1), (r"a\b", -4, 1), (r"\Ba", -4, 0), (r"\Aa", -4, 0), (r"a\Z", -4, 1), (r"(a)\1", -4, 3), (r"\0", -4, 0), (r"\a", -4, 0), (r"\u00e9", -4, 0),
    ("(?=a)", -4, 0), ("(?!a)", -4, 0), ("(?<=a)b", -4, 0), ("(?P<n>a)", -4, 0), ("(?i)a", -4, 0), ("(?#c)a", -4, 0), ("a*?", -4, 2), ("a+?", -4, 2), ("a??", -4, 2),
    ("a{1,2}?", -4, 6), ("a*+", -4, 2), ("a++", -4, 2), ("a{2}+", -4, 4), ("a{256}", -4, 1), ("a{0,300}", -4, 1), ("a{300,}", -4, 1), ("[é]", -4, 1), ("[a-é]", -4, 3),
    (r"[\b]", -4, 1), (r"\xff", -4, 0), (r"\x80", -4, 0), (r"[\x80]", -4, 1),
]


def test_every_refused_construct_has_its_code_and_offset_and_leaves_the_pool(libs):
    pkg, _, host = libs
    f = pkg.hostabi.Fsm(host, 4)
    with pytest.raises(pkg.hostabi.RegexError) as e:                     # no vocabulary yet: bad arguments
        f.add_regex("a")
    assert e.value.code == -1
    f.set_vocab([b"", b"a", b"b", b"ab"])
    assert f.add_stop([[1, 2]]) == 0 and f.add_regex("a+b", 0) == 3
    before, tables = f.n_states, [t.copy() for t in f.tables()]
    for p, code, off in REFUSED:
        with pytest.raises(pkg.hostabi.RegexError) as e:
            f.add_regex(p)
        assert (e.value.code, e.value.offset) == (code, off), (p, e.value.code, e.value.offset)
        assert f.n_states == before, p
        with pytest.raises(pkg.hostabi.RegexError) as e:
            pkg.hostabi.byte_dfa(host, p)
        assert (e.value.code, e.value.offset) == (code, off), p
    # more subset states than a pool has states; and a range that does not fit what is left of the pool
    with pytest.raises(pkg.hostabi.RegexError) as e:
        f.add_regex("(a|b)*a(a|b){16}")
    assert e.value.code == -2 and f.n_states == before
    for bad in (-2, 4):                                                  # an eos outside the vocabulary
        with pytest.raises(pkg.hostabi.RegexError) as e:
            f.add_regex("a", bad)
        assert e.value.code == -1 and f.n_states == before
    with pytest.raises(ValueError):
        f.set_vocab([b"", b"a", b"b", b"ab"])                            # not once a regex range exists
    for a, b in zip(tables, f.tables()):
        assert (a == b).all()
    # what every one of them is in Python: an error, or a construct re knows and this dialect leaves out
    for p, code, _ in REFUSED:
        if code == -4:
            continue
        if p in ("", "()", "(?:)", "a{", "a{x}", "a{,3}", "{2}"):          # (re reads these as empty matches or literals; refused here on purpose)
            continue
        with pytest.raises(re.error):
            re.compile(p, re.ASCII)
    f.close()


def test_equal_languages_give_equal_tables_and_state_counts_are_pinned(libs):
    pkg, _, host = libs
    dfa = lambda p: pkg.hostabi.byte_dfa(host, p)          # noqa: E731
    for a, b in [("a|b", "[ab]"), ("aa*", "a+"), ("(ab)?", "(?:ab|)"), ("a{2,}", "aaa*"), ("(a|b)*", "[ab]*"), ("abc|abd", "ab[cd]"), (r"\d", "[0-9]"),
                 ("a{0,2}", "(a(a)?)?"), ("(a*)*", "a*"), ("é|a", "a|é"), (".", r"[^\n]"), (r"\w", "[A-Za-z0-9_]"), ("x(a|b|c)", "x[a-c]")]:
        (na, aa), (nb, ab) = dfa(a), dfa(b)
        assert na.shape == nb.shape and (na == nb).all() and (aa == ab).all(), (a, b)
    for p, n in [("a", 2), ("a|b", 2), ("a+", 2), ("a{0}", 1), ("(ab)?", 3), ("a{3,}", 4), ("[0-9]{1,3}", 4), ("(a|b)*abb", 4), (".", 9), (r'\{"k": [0-9]{1,3}\}', 11),
                 ("abc|abd|ab", 4), ("(a|b)*a(a|b){3}", 16)]:
        assert len(dfa(p)[1]) == n, (p, len(dfa(p)[1]))
    # the numbering is breadth first from the start, bytes ascending: "b|ac" numbers the state behind a (byte 0x61) before the one behind b
    n256, acc = dfa("bd|ac")
    assert n256[0][ord("a")] == 1 and n256[0][ord("b")] == 2 and n256[1][ord("c")] == 3 and n256[2][ord("d")] == 3 and acc.tolist() == [0, 0, 0, 1]
    # "." is one state per UTF-8 continuation depth and lead class, and every edge leaves the start or goes on inside one code point
    n256, acc = dfa(".")
    assert acc.sum() == 1 and n256[0][ord("\n")] == ref.NONE and (n256[0][0x80:0xC2] == ref.NONE).all() and (n256[0][0xF5:] == ref.NONE).all()


THREE = [r"-?[0-9]{1,3}", r"(yes|no|maybe)( [a-z]+)?", r'\{"name": "[a-z]+", "age": [0-9]{1,3}\}']


def test_the_tokenizers_byte_strings(libs, vocab):
    pkg, _, host = libs
    vb, vo = vocab
    pieces = ref.pieces_of(vocab)
    t = host.tokenizer(VOCAB)
    assert len(pieces) == N_VOCAB and vo[0] == 0 and vo[-1] == len(vb) and (np.diff(vo) >= 0).all()
    assert pieces[0] == pieces[1] == pieces[2] == b"" and all(p == b"" for p in pieces[32000:])          # control pieces; ids past the tokenizer
    assert pieces[3] == b"\x00" and pieces[3 + 0x41] == b"A" and pieces[3 + 0xFF] == b"\xff"              # "<0xHH>" as the single byte, NUL too
    for i in (259, 260, 1000, 15043, 29871, 31999):
        assert pieces[i] == t.decode(0, i) and len(pieces[i]) >= 1, i                                    # as decode prints it, no dropped space
    assert pieces[29871] == b" " and any(p.startswith(b" ") and len(p) > 1 for p in pieces)
    none_empty = ref.pieces_of(t.vocab_bytes(N_VOCAB, empty=[]))
    assert none_empty[1] == t.decode(0, 1) and none_empty[1] != b"" and none_empty[32000] == b""
    mine = ref.pieces_of(t.vocab_bytes(300, empty=[5, 299, 70000]))
    assert len(mine) == 300 and mine[5] == mine[299] == b"" and mine[0] == t.decode(0, 0) and mine[6] == b"\x03"
    t.close()


@pytest.mark.parametrize("eos", [-1, 2])
def test_host_expansion_against_the_walk_over_the_vendored_vocabulary(libs, vocab, eos):
    pkg, hip, host = libs
    pieces = ref.pieces_of(vocab)
    f = pkg.hostabi.Fsm(host, N_VOCAB)
    f.set_vocab(vocab)
    stop = f.add_stop([[5, 6]])                                          # a host range in front, so that base > 0
    starts = [f.add_regex(p, eos) for p in THREE]
    assert f.add_regex(THREE[1], eos) == starts[1] and f.n_regex == 3    # an identical (pattern, eos) shares its range
    other = f.add_regex(THREE[1], 7 if eos < 0 else -1)                  # ... another eos does not
    assert other not in starts and f.n_regex == 4
    nxt, flags = f.tables()
    assert f.n_states == len(flags) and stop == 0 and starts[0] == 3
    assert hip.fsm_check(nxt, flags, N_VOCAB) == (0, -1)
    g = np.random.default_rng(5)
    for p, base in zip(THREE, starts):
        n256, acc = pkg.hostabi.byte_dfa(host, p)
        rows, fl = ref.expand(n256, acc, pieces, eos, base)
        S = len(fl)
        assert (nxt[base:base + S] == rows).all() and (flags[base:base + S] == fl).all(), p
        assert (nxt[base:base + S, [0, 1, 32000, 32001]] == ref.DEAD).all()                                 # empty pieces are DEAD
        if eos >= 0:
            live = [s for s in range(len(acc)) if acc[s] and (n256[s] != ref.NONE).any()]
            assert (len(live) >= 1 or p == THREE[2]) and all(nxt[base + s][eos] == base + len(acc) for s in live)           # may stop here or go on: eos enters END
            assert all(nxt[base + s][eos] == ref.DEAD for s in range(len(acc)) if s not in live)         # eos is dead everywhere else
            assert flags[base + len(acc)] == 1 and (nxt[base + len(acc)] == ref.DEAD).all()              # END: final, its row dead
            assert not any(flags[base + s] for s in live)
        # sampled walks over the token table (fixed seed; half the steps prefer an id that leaves the state, so that loops end): the
        # token state is the byte automaton's state on the text so far, and the text is one re accepts exactly where that state accepts --
        # so whatever id string the table accepts decodes to a string re accepts
        rx, done = re.compile(p, re.ASCII), 0
        for _ in range(60):
            s, text = base, b""
            for _ in range(200):
                if flags[s]:
                    break
                allowed = np.flatnonzero(nxt[s] != ref.DEAD)
                away = allowed[nxt[s][allowed] != s]
                i = int(g.choice(away if len(away) and g.integers(0, 2) else allowed))
                text += pieces[i]
                s = int(nxt[s][i])
            bs = 0
            for c in text:
                bs = int(n256[bs][c])
                assert bs != ref.NONE, (p, text)
            assert s - base in (bs, len(acc)) and ((s - base == len(acc)) <= bool(acc[bs])), (p, text)
            assert bool(acc[bs]) == (rx.fullmatch(text.decode()) is not None), (p, text)
            if flags[s]:
                done += 1
                assert rx.fullmatch(text.decode()) is not None, (p, text)
        assert done >= 10 or (eos < 0 and p == THREE[1]), (p, done)          # (without an eos that pattern never reaches a final state)
    f.close()


def test_a_state_no_piece_can_leave_is_stuck(libs):
    pkg, hip, host = libs
    f = pkg.hostabi.Fsm(host, 3)
    f.set_vocab([b"", b"a", b"b"])
    s = f.add_regex("ac")                                                # no piece spells c: the state behind a allows no id
    nxt, flags = f.tables()
    assert hip.fsm_check(nxt, flags, 3) == (4, s + 1)
    f.close()
    f = pkg.hostabi.Fsm(host, 3)
    f.set_vocab([b"", b"a", b"b"])
    f.add_regex("a*")                                                    # eos -1: the accepting start goes on for ever, and may
    nxt, flags = f.tables()
    assert hip.fsm_check(nxt, flags, 3) == (0, -1) and flags.tolist() == [0] and nxt.tolist() == [[ref.DEAD, 0, ref.DEAD]]
    f.close()


def test_regex_code_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """tests/host_sanitize_regex.cpp: a stand-alone program (its own main, nothing loaded into Python) that compiles and expands a list
    of patterns, good and refused ones, through host/regex_build.h and host/fsm_build.h"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "host_sanitize_regex")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tinyllama.cpp_amd"), os.path.join(ROOT, "tests", "host_sanitize_regex.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:protect_shadow_gap=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    assert "host_sanitize_regex ok" in r.stdout


def test_the_command_line_refuses_what_it_cannot_bind(libs):
    """--regex is refused beside --choice and beside --stop (an answer is bound to one start state of one automaton), beside --ban /
    --allow and --score, without its value, and with a pattern the compiler refuses -- all before any file is opened"""
    pkg, _, _ = libs
    cli = pkg.build.HOST_CLI
    for args, what in [(["--regex", "a", "--choice", "5"], "--regex and --choice"), (["--stop", "5", "--regex", "a"], "--regex and --stop"),
                       (["--regex", "a", "--ban", "5"], "--ban"), (["--regex", "a", "--score", "x.txt"], "--score"), (["--regex"], "regex value is missing"),
                       (["--regex", "a(?=b)"], "unsupported construct at byte 1"), (["--regex", "(a"], "bad syntax at byte 0")]:
        r = subprocess.run([cli, *args], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and what in r.stderr, (args, r.stderr[-400:])
    r = subprocess.run([cli, "--regex", "[a-z]+", "--model", "/nonexistent/x.gten", "-p", "hi"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "cannot open the checkpoint" in r.stderr                     # a good pattern gets as far as the files
    assert "--regex PATTERN" in subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60).stdout
