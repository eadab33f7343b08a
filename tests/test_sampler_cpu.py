"""not gpu: the top-k sampler's restatement (tests/sample_ref.py) and the new C-ABI headers (include/gten_hip_sample.h,
include/gten_host_sample.h): exported by the libraries and bound in the Python wrappers."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sample_ref as ref  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402
from test_abi_loads import declared_symbols  # noqa: E402


def test_philox_known_answers():
    """Random123's known-answer vectors for philox4x32-10 (word 0)"""
    assert int(ref.philox4x32((0, 0, 0, 0), (0, 0))[0]) == 0x6627E8D5
    assert int(ref.philox4x32((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2)[0]) == 0x408F276D
    assert int(ref.philox4x32((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))[0]) == 0xD16CFE09


def test_restatement_rules():
    x = np.array([1.0, 3.0, 3.0, 2.0, 3.0, -1.0], np.float32)
    assert ref.candidates(x, 2).tolist() == [1, 2]                  # ties at the threshold: the lower indices
    assert ref.candidates(x, 4).tolist() == [1, 2, 3, 4]
    assert ref.candidates(x, 99).tolist() == list(range(6))
    assert ref.draw(x, 0, 1.0, 1, 0, 5)[0] == 1                       # greedy: first maximum
    for s in range(20):
        assert ref.draw(x, 1, 0.01 + s, s, s, s)[0] == 1              # top_k 1: greedy at any temperature
    u = ref.uniform(np.arange(4096), 7, 3, 0xDEADBEEF12345678)
    assert (u > 0).all() and (u < 1).all() and u.dtype == np.float32


def test_sample_headers_are_exported_and_bound():
    pkg = load_package()
    pkg.build.build_all()
    api = pkg.hipabi.GtenHip()
    names = declared_symbols("gten_hip_sample.h")
    assert sorted(api.SAMPLE_SYMBOLS) == names and len(names) == 2
    assert not set(names) & set(declared_symbols("gten_hip.h"))
    for name in names:
        assert hasattr(api.lib, name), name
    host = pkg.hostabi.GtenHost()
    names = declared_symbols("gten_host_sample.h")
    assert sorted(host.SAMPLE_SYMBOLS) == names and len(names) == 3
    for name in names:
        assert hasattr(host.lib, name), name
    assert api.prof_family_index("decode_sample") >= 0              # the sampler's launches are a family of their own


def test_sampled_serve_under_sanitizers_against_a_stub_device(tmp_path):
    """host/capi_sample.cpp's sampled serve under ASan + UBSan over tests/hip_stub.cpp + tests/hip_stub_sample.cpp (the sampler
    restated on the CPU, set_sampling recorded): top_k 1 gives the greedy serve's ids, and every admitted prompt's request
    reached its slot"""
    import shutil
    import subprocess
    import pytest
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "host_sanitize_sample")
    host = os.path.join(ROOT, "tinyllama.cpp_amd", "host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fopenmp", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tinyllama.cpp_amd"),
           os.path.join(ROOT, "tests", "host_sanitize_sample.cpp"), os.path.join(ROOT, "tests", "hip_stub.cpp"),
           os.path.join(ROOT, "tests", "hip_stub_sample.cpp"), os.path.join(host, "capi.cpp"), os.path.join(host, "capi_sample.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:protect_shadow_gap=0", UBSAN_OPTIONS="print_stacktrace=1", OMP_NUM_THREADS="2")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    assert "host_sanitize_sample ok" in r.stdout


def test_sample_stub_covers_the_whole_header(tmp_path):
    import shutil
    import subprocess
    import ctypes
    import pytest
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    so = str(tmp_path / "libhip_stub_sample.so")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "hip_stub_sample.cpp"), "-o", so], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = ctypes.CDLL(so)
    for name in declared_symbols("gten_hip_sample.h"):
        assert hasattr(lib, name), name
