"""not gpu: the entry points behind "decode slots that share a prefix read one copy of its K / V"
(include/gten_hip_prefix_decode.h, include/gten_host_prefix_decode.h) are exported by the two libraries, declared by the headers
and bound by the Python side; include/gten_hip.h and include/gten_hip_prefix.h do not grow by them, and host/capi.cpp with the
headers it instantiates reaches them through hooks only (it must go on linking against tests/hip_stub.cpp alone)."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from __graft_entry__ import load_package  # noqa: E402
from test_abi_loads import declared_symbols  # noqa: E402

HIP_NAMES = ["gten_hip_decoder_prefix_info", "gten_hip_decoder_prefix_set", "gten_hip_decoder_slot_share", "gten_hip_set_prefix_decode_shared"]
HOST_NAMES = ["gten_host_batch_prefix_decode_info", "gten_host_batch_prefix_decode_share", "gten_host_set_prefix_decode_shared"]


def test_hip_library_exports_the_prefix_decode_header():
    pkg = load_package()
    pkg.build.build_hip()
    api = pkg.hipabi.GtenHip()
    names = declared_symbols("gten_hip_prefix_decode.h")
    assert names == HIP_NAMES
    for name in names:
        assert hasattr(api.lib, name), f"{name} declared in include/gten_hip_prefix_decode.h but not exported"
    assert sorted(api.PREFIX_DECODE_SYMBOLS) == names, "python binding out of sync with the header"
    assert callable(api.set_prefix_decode_shared)


def test_host_library_exports_the_prefix_decode_header():
    pkg = load_package()
    pkg.build.build_all()
    host = pkg.hostabi.GtenHost()
    names = declared_symbols("gten_host_prefix_decode.h")
    assert names == HOST_NAMES
    for name in names:
        assert hasattr(host.lib, name), f"{name} declared in include/gten_host_prefix_decode.h but not exported"
    assert sorted(host.PREFIX_DECODE_SYMBOLS) == names
    assert callable(pkg.hostabi.HostBatch.prefix_decode_info) and callable(pkg.hostabi.HostBatch.prefix_decode_share_rc)
    assert callable(pkg.hostabi.GtenHost.set_prefix_decode_shared)


def test_only_the_prefix_translation_unit_names_the_device_entry_points():
    pkg = load_package()
    assert not set(pkg.hipabi.GtenHip.PREFIX_DECODE_SYMBOLS) & set(pkg.hipabi.GtenHip.SYMBOLS + pkg.hipabi.GtenHip.PREFIX_SYMBOLS)
    main = open(os.path.join(ROOT, "include", "gten_hip.h")).read()
    pat = re.compile(r"\b(%s)\b" % "|".join(HIP_NAMES))
    assert not pat.search(main)
    host_dir = os.path.join(ROOT, "tinyllama.cpp_amd")
    for base, _, files in os.walk(host_dir):
        if os.path.basename(base) == "csrc":
            continue                                   # (the library that defines them)
        for f in files:
            if not f.endswith((".h", ".cpp")) or f == "capi_prefix.cpp":
                continue
            text = re.sub(r"//[^\n]*|/\*.*?\*/", "", open(os.path.join(base, f), errors="replace").read(), flags=re.S)
            assert not pat.search(text), os.path.join(base, f)
