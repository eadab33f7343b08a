"""not gpu: the 4-bit K / V shadows' arithmetic and layout without a device.  csrc/gten_kvq4_math.h -- the text the
kernels compile -- in a stand-alone program under ASan + UBSan (tests/host_kvq4_math.cpp): R idempotent over every f16 delta, the
chunk's offset functions bijections; the same header against the NumPy restatement on the GPU tests' rows; the new headers bound."""
import os
import re
import subprocess

import numpy as np
import pytest

import kv_q4_ref as ref
from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "host_kvq4_math.cpp")
    assert [line for line in open(src) if line.startswith('#include "')] == ['#include "../tinyllama.cpp_amd/csrc/gten_kvq4_math.h"\n']
    math_h = open(os.path.join(ROOT, "tinyllama.cpp_amd", "csrc", "gten_kvq4_math.h")).read()
    assert [line for line in math_h.split("\n") if line.startswith("#include")] == ["#include <math.h>", "#include <stdint.h>"] and "hip/" not in math_h
    exe = str(tmp_path_factory.mktemp("kvq4") / "host_kvq4_math")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", src, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_idempotence_sweep_and_layout_bijections(program):
    r = subprocess.run([program], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "host_kvq4_math ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


@pytest.mark.parametrize("n_rows,n_blocks,seed", [(37, 5, 11), (64, 8, 2), (3, 1, 5)])
def test_shared_header_is_the_restatement(program, tmp_path, n_rows, n_blocks, seed):
    rows = ref.edge_rows(n_rows, n_blocks, seed)
    rows.tofile(tmp_path / "in.bin")
    assert subprocess.run([program, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], timeout=600).returncode == 0
    got = np.fromfile(tmp_path / "out.bin", np.uint8).reshape(rows.shape)
    want = ref.round_rows(rows)
    assert np.array_equal(got, want)
    assert np.array_equal(ref.round_rows(want), want) and not np.array_equal(want, rows)


def test_new_headers_are_exported_and_bound():
    pkg = load_package()
    pkg.build.build_all()
    for header, api, names in (("gten_hip_kvq4.h", pkg.hipabi.GtenHip(), pkg.hipabi.GtenHip.KVQ4_SYMBOLS),
                               ("gten_host_kvq4.h", pkg.hostabi.GtenHost(), pkg.hostabi.GtenHost.KVQ4_SYMBOLS)):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        declared = sorted(set(re.findall(r"\b(gten_(?:hip|host)_[a-z0-9_]+)\s*\(", text)))
        assert declared == sorted(names), header
        for name in names:
            assert hasattr(api.lib, name), name
    assert all(callable(getattr(pkg.hostabi.HostBatch, m)) for m in ("kv_round_q4", "kv_shadow_info", "kv_shadow_read"))
    assert callable(pkg.hipabi.GtenHip.set_kv_shadow_q4) and callable(pkg.hipabi.GtenHip.kv_round_q4)
