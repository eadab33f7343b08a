"""not gpu: continued rows and continued sequences (include/gten_hip_continue.h, include/gten_host_sessions.h) are
exported by the two libraries and bound by the Python side; the prefix headers keep exactly their symbols; only
host/capi_sessions.cpp names the device entry points (host/capi.cpp goes on linking against tests/hip_stub.cpp alone); and
the exported turn plan agrees with tests/sessions_ref.py."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from __graft_entry__ import load_package  # noqa: E402
from test_abi_loads import declared_symbols  # noqa: E402
import sessions_ref  # noqa: E402

HIP_NAMES = ["gten_hip_block_rows_continued", "gten_hip_set_row_contexts"]
HOST_NAMES = sorted(["gten_host_batch_extend_info", "gten_host_batch_extend_many", "gten_host_session_plan", "gten_host_batch_sessions_reserve",
                     "gten_host_batch_session_open", "gten_host_batch_session_close", "gten_host_batch_session_info", "gten_host_batch_session_ids",
                     "gten_host_batch_session_truncate", "gten_host_batch_sessions_info", "gten_host_batch_serve_sessions"])


def test_hip_library_exports_the_continue_header():
    pkg = load_package()
    pkg.build.build_hip()
    api = pkg.hipabi.GtenHip()
    names = declared_symbols("gten_hip_continue.h")
    assert names == HIP_NAMES
    for name in names:
        assert hasattr(api.lib, name), f"{name} declared in include/gten_hip_continue.h but not exported"
    assert sorted(api.CONTINUE_SYMBOLS) == names, "python binding out of sync with the header"
    assert callable(api.set_row_contexts) and callable(api.block_rows_continued)
    assert not set(api.CONTINUE_SYMBOLS) & set(api.SYMBOLS)
    text = open(os.path.join(ROOT, "include", "gten_hip.h")).read()
    assert "continued" not in text and "row_ctx" not in text


def test_host_library_exports_the_sessions_header():
    pkg = load_package()
    pkg.build.build_all()
    host = pkg.hostabi.GtenHost()
    names = declared_symbols("gten_host_sessions.h")
    assert names == HOST_NAMES
    for name in names:
        assert hasattr(host.lib, name), f"{name} declared in include/gten_host_sessions.h but not exported"
    assert sorted(host.SESSIONS_SYMBOLS) == names
    assert not set(host.SESSIONS_SYMBOLS) & set(host.SYMBOLS)
    assert callable(pkg.hostabi.HostBatch.extend_many) and callable(pkg.hostabi.HostBatch.extend_info) and callable(host.session_plan)
    for name in ("sessions_reserve", "session_open", "session_close", "session_info", "session_ids", "session_truncate", "sessions_info", "serve_sessions"):
        assert callable(getattr(pkg.hostabi.HostBatch, name)), name
    assert host.SESSIONS_MAX == 256 and "#define GTEN_HOST_SESSIONS_MAX 256" in open(os.path.join(ROOT, "include", "gten_host_sessions.h")).read()


def test_the_prefix_headers_keep_their_symbols():
    assert declared_symbols("gten_hip_prefix.h") == ["gten_hip_block_rows_prefixed"]
    assert declared_symbols("gten_host_prefix.h") == ["gten_host_batch_prefix_info", "gten_host_batch_set_prefix"]


def test_only_capi_sessions_names_the_device_entry_points():
    pat = re.compile(r"\b(" + "|".join(HIP_NAMES) + r")\b")
    seen = False
    for base, _, files in os.walk(os.path.join(ROOT, "tinyllama.cpp_amd")):
        if os.path.basename(base) == "csrc":
            continue                                             # (the library that defines them)
        for f in files:
            if not f.endswith((".h", ".cpp")):
                continue
            text = re.sub(r"//[^\n]*|/\*.*?\*/", "", open(os.path.join(base, f), errors="replace").read(), flags=re.S)
            if f == "capi_sessions.cpp":
                seen = all(n in text for n in HIP_NAMES)
                continue
            assert not pat.search(text), os.path.join(base, f)
    assert seen, "host/capi_sessions.cpp installs both entry points"
    # the stub that stands in for include/gten_hip.h does not grow by them either
    assert not pat.search(open(os.path.join(ROOT, "tests", "hip_stub.cpp")).read())


def test_session_plan_agrees_with_the_reference():
    pkg = load_package()
    pkg.build.build_all()
    host = pkg.hostabi.GtenHost()
    cases = sessions_ref.cases(200)
    assert len(cases) == 200
    seen = set()
    for h, r, n_new, seg in cases:
        want = sessions_ref.plan(h, r, n_new, seg)
        got = host.session_plan(h, r, n_new, seg)
        assert got == want, (h, r, n_new, seg, got, want)
        if want is None:
            continue
        ctx, k, path = want
        assert k >= 1 and ctx + k == h + n_new and 0 <= ctx <= r
        seen |= {("h0", h == 0), ("r=h", r == h and h > 0), ("empty", n_new == 0), ("k", k if k in (15, 16) else 0), ("path", path)}
    for need in (("h0", True), ("r=h", True), ("empty", True), ("k", 15), ("k", 16), ("path", 0), ("path", 1), ("path", 2)):
        assert need in seen, need
    # k = 15 (a filled segment) and k = 16 are continued segments -- unless prompts are not processed as segments
    assert host.session_plan(100, 99, 14) == (99, 15, sessions_ref.CONTINUED)
    assert host.session_plan(100, 99, 15) == (99, 16, sessions_ref.CONTINUED)
    assert host.session_plan(100, 99, 15, segmented=False) == (99, 16, sessions_ref.ONE_BY_ONE)
    # a conversation of fewer than 16 ids in all stays with the operators, as such a prompt does
    assert host.session_plan(10, 10, 5) == (10, 5, sessions_ref.ONE_BY_ONE)
    assert host.session_plan(10, 10, 6) == (10, 6, sessions_ref.CONTINUED)
    # an empty turn behind a full history computes the last row again: there is always a row to take logits from
    assert host.session_plan(40, 40, 0) == (39, 1, sessions_ref.CONTINUED)
