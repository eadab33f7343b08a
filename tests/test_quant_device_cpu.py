"""not gpu: the device quantiser's device-free side: the two new headers against their QUANT_SYMBOLS lists and
the exports, their names disjoint from every older list, and the command line's refusal of --from-f16 with -f16."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from __graft_entry__ import load_package  # noqa: E402
from test_abi_loads import declared_symbols  # noqa: E402


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    p.build.build_all()
    return p


@pytest.mark.parametrize("side, header", [("hipabi.GtenHip", "gten_hip_quant.h"), ("hostabi.GtenHost", "gten_host_quant.h")])
def test_quant_header_is_its_list_exported_and_disjoint(pkg, side, header):
    mod, cls = side.split(".")
    api = getattr(getattr(pkg, mod), cls)()
    names = declared_symbols(header)
    assert names and sorted(api.QUANT_SYMBOLS) == names
    for name in names:
        assert hasattr(api.lib, name), name
    for attr in dir(api):
        if attr.endswith("SYMBOLS") and attr != "QUANT_SYMBOLS":
            assert not set(names) & set(getattr(api, attr)), attr
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != header:
            assert not set(names) & set(declared_symbols(other)), other


@pytest.mark.parametrize("args", [("--from-f16", "-f16"), ("-f16", "--from-f16"), ("--from-f16",)])
def test_cli_refuses_from_f16_in_an_f16_model(pkg, args):
    r = subprocess.run([pkg.build.HOST_CLI, *args, "--model", "/nonexistent/m.gten"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--from-f16" in r.stderr and "-f16" in r.stderr and "cannot open" not in r.stderr, r.stderr[-300:]
    ok = subprocess.run([pkg.build.HOST_CLI, "--from-f16", "-q4", "--model", "/nonexistent/m.gten"], capture_output=True, text=True, timeout=120)
    assert ok.returncode != 0 and "cannot open the checkpoint" in ok.stderr, ok.stderr[-300:]
