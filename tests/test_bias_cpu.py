"""not gpu: the bias tables' restatement (tests/bias_ref.py), the new C-ABI headers (include/gten_hip_bias.h,
include/gten_host_bias.h: exported by the libraries and bound in the Python wrappers) and the command line's --ban / --allow /
--min-new refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bias_ref as bref  # noqa: E402
import sample_ref as ref  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402
from test_abi_loads import declared_symbols  # noqa: E402


def row(n, seed):
    return (np.random.default_rng(seed).standard_normal(n) * 2.0).astype(np.float32)


def test_empty_table_is_the_plain_draw():
    x = row(97, 1)
    b = bref.table(97)
    for s in range(50):
        for k in (0, 1, 5, 97, 200):
            assert bref.draw(x, b, k, 0.9, s, 3, 10 + s) == ref.draw(x, k, 0.9, s, 3, 10 + s)
    # a table that has run out (position >= until) is no table; one that has not is
    banned = int(np.argmax(x))
    b = bref.table(97, [(banned, -np.inf)])
    assert bref.draw(x, b, 0, 1.0, 0, 0, 7, until=7)[0] == banned
    assert bref.draw(x, b, 0, 1.0, 0, 0, 6, until=7)[0] != banned
    assert bref.draw(x, b, 0, 1.0, 0, 0, 7000, until=0)[0] != banned


def test_a_banned_id_is_never_drawn():
    """10 000 seeds, the banned id the row's maximum by a wide margin: without the table it wins nearly every draw"""
    x = row(24, 2)
    banned = 5
    x[banned] = x.max() + 6.0
    b = bref.table(24, [(banned, -np.inf)])
    plain = 0
    for s in range(10000):
        k = (0, 1, 3, 24, 40)[s % 5]
        assert bref.draw(x, b, k, 1.3, s, s % 7, 1 + s % 300)[0] != banned, s
        plain += ref.draw(x, k, 1.3, s, s % 7, 1 + s % 300)[0] == banned
    assert plain > 9000


def test_one_allowed_id_is_always_drawn():
    x = row(64, 3)
    for only in (0, 17, 63):
        b = bref.table(64, allow=[only])
        assert bref.allowed(b).tolist() == [only]
        for s in range(200):
            for k in (0, 1, 2, 40, 64, 100):
                assert bref.draw(x, b, k, 0.7, s, 1, 5 + s)[0] == only


def test_top_k_above_the_allowed_count_is_the_allowed_count():
    x = row(200, 4)
    allow = [3, 50, 51, 120, 199]
    b = bref.table(200, [(50, 2.5), (120, -1.0)], allow=allow)
    for s in range(300):
        want = bref.draw(x, b, len(allow), 0.9, s, 2, 9 + s)
        assert want[0] in allow
        for k in (len(allow) + 1, 40, 200, 1000):
            assert bref.draw(x, b, k, 0.9, s, 2, 9 + s) == want, (s, k)
    assert len({bref.draw(x, b, 40, 0.9, s, 2, 9)[0] for s in range(300)}) > 1       # (it is a draw, not one id)


def test_table_requests():
    assert bref.table_ok(10) and bref.table_ok(10, [(3, -np.inf)]) and bref.table_ok(10, [(3, 0.0)], fill=-np.inf)
    assert bref.table_ok(10, [(0, 1e30), (1, -1e30)])
    assert not bref.table_ok(10, [(10, 0.0)]) and not bref.table_ok(10, [(-1, 0.0)])       # id outside the vocabulary
    assert not bref.table_ok(10, [(3, 0.0), (3, 1.0)])                                     # repeated id
    assert not bref.table_ok(10, [(3, np.nan)]) and not bref.table_ok(10, [(3, np.inf)]) and not bref.table_ok(10, [(3, 2e30)])
    assert not bref.table_ok(10, fill=-np.inf) and not bref.table_ok(10, [(j, -np.inf) for j in range(10)])   # every id banned
    assert not bref.table_ok(10, fill=np.nan)


def test_bias_headers_are_exported_and_bound():
    pkg = load_package()
    pkg.build.build_all()
    api = pkg.hipabi.GtenHip()
    names = declared_symbols("gten_hip_bias.h")
    assert sorted(api.BIAS_SYMBOLS) == names and len(names) == 4
    assert not set(names) & set(declared_symbols("gten_hip.h")) and not set(names) & set(declared_symbols("gten_hip_sample.h"))
    for name in names:
        assert hasattr(api.lib, name), name
    host = pkg.hostabi.GtenHost()
    names = declared_symbols("gten_host_bias.h")
    assert sorted(host.BIAS_SYMBOLS) == names and len(names) == 11
    for name in names:
        assert hasattr(host.lib, name), name
    header = open(os.path.join(ROOT, "include", "gten_hip_bias.h")).read()
    assert f"#define GTEN_HIP_BIAS_TABLES {api.BIAS_TABLES}\n" in header and api.BIAS_TABLES >= 16 and bref.TABLES == api.BIAS_TABLES


def test_python_table_shorthand():
    pkg = load_package()
    ids, values, fill = pkg.hostabi.bias_pairs([(3, -np.inf), (9, 1.5)])
    assert ids.tolist() == [3, 9] and values.tolist() == [-np.inf, 1.5] and fill == 0.0
    ids, values, fill = pkg.hostabi.bias_pairs(allow=[4, 2], pairs=[(2, 0.5)])
    assert dict(zip(ids.tolist(), values.tolist())) == {4: 0.0, 2: 0.5} and fill == -np.inf
    with pytest.raises(ValueError):
        pkg.hostabi.bias_pairs(allow=[4, 4])
    with pytest.raises(ValueError):
        pkg.hostabi.bias_pairs(allow=[4], pairs=[(5, 1.0)])


@pytest.fixture(scope="module")
def cli():
    pkg = load_package()
    pkg.build.build_all()
    return pkg.build.HOST_CLI


def run(cli, *args):
    return subprocess.run([cli, *args], capture_output=True, text=True, timeout=120)


def test_cli_refuses_bad_constraints(cli):
    """every refusal comes from the option parser, before a checkpoint is opened"""
    for args, said in ((("--ban", "abc"), "Invalid ban value"), (("--ban", "1,,2"), "Invalid ban value"), (("--ban", ""), "Invalid ban value"),
                       (("--ban", "1,2x"), "Invalid ban value"), (("--ban", "32003"), "ban ids must be"), (("--ban", "-1"), "ban ids must be"),
                       (("--ban", "7,7"), "twice"), (("--allow", "x"), "Invalid allow value"), (("--allow", "40000"), "allow ids must be"),
                       (("--allow", "5,6,5"), "twice"), (("--min-new", "0", "--ban", "3"), "min-new must be"),
                       (("--min-new", "abc", "--ban", "3"), "Invalid min-new value"), (("--min-new", "4"), "min-new needs"),
                       (("--allow", "5,6", "--ban", "6,5"), "bans every id"), (("--ban",), "value is missing")):
        r = run(cli, *args)
        assert r.returncode != 0 and said in r.stderr and "cannot open" not in r.stderr, (args, r.stderr[-300:])
    r = run(cli, "--help")
    assert r.returncode == 0 and "--ban" in r.stdout and "--allow" in r.stdout and "--min-new" in r.stdout
    # well-formed constraints pass the parser: the next complaint is the missing checkpoint
    r = run(cli, "--ban", "2,0,31999", "--allow", "5,6,7", "--min-new", "3", "--model", "/nonexistent/m.gten")
    assert r.returncode != 0 and "cannot open the checkpoint" in r.stderr
