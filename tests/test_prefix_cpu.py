"""not gpu: the shared-prefix entry points (include/gten_hip_prefix.h, include/gten_host_prefix.h) are exported by the two
libraries and bound by the Python side; include/gten_hip.h does not grow by them (tests/hip_stub.cpp stands in for every
symbol THAT header declares, and host/capi.cpp must go on linking against the stub alone)."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from __graft_entry__ import load_package  # noqa: E402
from test_abi_loads import declared_symbols  # noqa: E402


def test_hip_library_exports_the_prefix_header():
    pkg = load_package()
    pkg.build.build_hip()
    api = pkg.hipabi.GtenHip()
    names = declared_symbols("gten_hip_prefix.h")
    assert names == ["gten_hip_block_rows_prefixed"]
    for name in names:
        assert hasattr(api.lib, name), f"{name} declared in include/gten_hip_prefix.h but not exported"
    assert sorted(api.PREFIX_SYMBOLS) == names, "python binding out of sync with the header"
    assert callable(api.block_rows_prefixed)


def test_host_library_exports_the_prefix_header():
    pkg = load_package()
    pkg.build.build_all()
    host = pkg.hostabi.GtenHost()
    names = declared_symbols("gten_host_prefix.h")
    assert names == ["gten_host_batch_prefix_info", "gten_host_batch_set_prefix"]
    for name in names:
        assert hasattr(host.lib, name), f"{name} declared in include/gten_host_prefix.h but not exported"
    assert sorted(host.PREFIX_SYMBOLS) == names
    assert callable(pkg.hostabi.HostBatch.set_prefix) and callable(pkg.hostabi.HostBatch.prefix_info)


def test_the_main_header_and_what_links_against_the_stub_do_not_name_the_new_entry_point():
    pkg = load_package()
    assert "prefixed" not in open(os.path.join(ROOT, "include", "gten_hip.h")).read()
    assert not set(pkg.hipabi.GtenHip.PREFIX_SYMBOLS) & set(pkg.hipabi.GtenHip.SYMBOLS)
    # host/capi.cpp and the headers it instantiates reach the entry point through a hook only: the one translation unit
    # that names the symbol is host/capi_prefix.cpp
    pat = re.compile(r"\bgten_hip_block_rows_prefixed\b")
    for base, _, files in os.walk(os.path.join(ROOT, "tinyllama.cpp_amd")):
        for f in files:
            if not f.endswith((".h", ".cpp")) or f == "capi_prefix.cpp":
                continue
            text = re.sub(r"//[^\n]*|/\*.*?\*/", "", open(os.path.join(base, f), errors="replace").read(), flags=re.S)
            assert not pat.search(text), os.path.join(base, f)
