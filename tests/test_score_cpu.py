"""not gpu: the scoring headers (include/gten_hip_score.h, include/gten_host_score.h) are exported by the libraries and
bound in the Python wrappers, the row kernel has a profiler family of its own, and the command line documents --score."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from __graft_entry__ import load_package  # noqa: E402
from test_abi_loads import declared_symbols  # noqa: E402


def test_score_headers_are_exported_and_bound():
    pkg = load_package()
    pkg.build.build_all()
    api = pkg.hipabi.GtenHip()
    names = declared_symbols("gten_hip_score.h")
    assert names == sorted(api.SCORE_SYMBOLS) == ["gten_hip_row_logprobs"]
    for name in names:
        assert hasattr(api.lib, name)
    host = pkg.hostabi.GtenHost()
    names = declared_symbols("gten_host_score.h")
    assert names == sorted(host.SCORE_SYMBOLS) and len(names) == 3
    for name in names:
        assert hasattr(host.lib, name)
    assert api.prof_family_index("row_logprobs") >= 0


def test_cli_usage_mentions_score_and_ctx():
    pkg = load_package()
    pkg.build.build_all()
    r = subprocess.run([pkg.build.HOST_CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--score PATH" in r.stdout and "--ctx N" in r.stdout
    for bad in ("16", "2049", "x"):
        r = subprocess.run([pkg.build.HOST_CLI, "--score", "nothing.txt", "--ctx", bad], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "ctx" in r.stderr
