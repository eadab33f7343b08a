"""not gpu: the context shift's device-free side.  The plan (host/shift_plan.h, exported as gten_host_shift_plan)
against a restatement in Python over a grid; the plan header alone under ASan + UBSan (tests/host_shift_plan.cpp, a stand-alone
program); the symbols of include/gten_hip_shift.h and include/gten_host_shift.h exported and bound; the numpy reference's swaps."""
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

import shift_ref as ref  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402


def host():
    pkg = load_package()
    pkg.build.build_all()
    return pkg.hostabi.GtenHost()


def plan_py(n_ids, rows, max_ctx, keep, drop):
    """the plan restated: a shift is due before the step that would write row max_ctx; drop 0 is half of what lies behind keep"""
    def resolve(r):
        return drop if drop > 0 else max((r - keep) // 2, 1)
    if n_ids < 0 or rows < 0 or rows > n_ids or max_ctx < 1 or rows > max_ctx or keep < 0 or drop < 0 or keep + resolve(max_ctx) > max_ctx:
        return None
    if rows < max_ctx:
        return (0, keep, 0, n_ids, rows)
    d = resolve(rows)
    return (1, keep, d, n_ids - d, rows - d)


def test_plan_agrees_with_its_restatement_over_a_grid():
    h = host()
    n = 0
    for max_ctx in (1, 2, 8, 64, 128, 2048):
        for keep in (-1, 0, 1, 4, 7, 63, 64, 100, 2047):
            for drop in (-2, 0, 1, 8, 57, 64, 2048):
                for rows in (-1, 0, 1, 5, max_ctx - 1, max_ctx, max_ctx + 1):
                    for n_ids in (rows - 1, rows, rows + 1, rows + 9):
                        assert h.shift_plan(n_ids, rows, max_ctx, keep, drop) == plan_py(n_ids, rows, max_ctx, keep, drop), (n_ids, rows, max_ctx, keep, drop)
                        n += 1
    assert n > 5000
    assert h.shift_plan(65, 64, 64, 4, 0) == (1, 4, 30, 35, 34)
    assert h.shift_plan(2049, 2048, 2048, 64, 0) == (1, 64, 992, 1057, 1056)
    assert h.shift_plan(64, 63, 64, 4, 0) == (0, 4, 0, 64, 63)


def test_phi_and_ids_follow_one_map():
    h = host()
    for n, keep, drop in ((3, 0, 1), (17, 1, 3), (300, 16, 100), (40, 4, 36), (64, 4, 30)):
        ids = list(range(500, 500 + n + 1))
        new = ref.shift_ids(ids, keep, drop)
        assert len(new) == n + 1 - drop
        for p in range(n + 1):
            q = h.shift_phi(p, keep, drop)
            assert q == ref.phi(p, keep, drop)
            if p < keep or p >= keep + drop:
                assert new[q] == ids[p]
            else:
                assert q == keep
    assert h.shift_drop(10, 0, 0) == 5 and h.shift_drop(10, 9, 0) == 1 and h.shift_drop(10, 8, 3) == -1 and h.shift_drop(10, 4, 3) == 3


def test_shift_plan_under_sanitizers(tmp_path):
    """the plan over a grid, phi and the ids, shifts chained through a thousand steps (tests/host_shift_plan.cpp), under ASan + UBSan.
    The program includes host/shift_plan.h alone, and that header is device-free."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = os.path.join(ROOT, "tests", "host_shift_plan.cpp")
    includes = [line for line in open(src) if line.startswith("#include \"")]
    assert includes == ['#include "../tinyllama.cpp_amd/host/shift_plan.h"\n'], includes
    plan = open(os.path.join(ROOT, "tinyllama.cpp_amd", "host", "shift_plan.h")).read()
    assert "#include" not in plan and "gten_hip" not in plan             # device-free: not even the standard library
    exe = str(tmp_path / "host_shift_plan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           src, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:protect_shadow_gap=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    assert "host_shift_plan ok" in r.stdout


def declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gten_(?:hip|host)_[a-z0-9_]+)\s*\(", text)))


def test_new_headers_are_exported_and_bound():
    pkg = load_package()
    pkg.build.build_all()
    api, h = pkg.hipabi.GtenHip(), pkg.hostabi.GtenHost()
    names = declared("gten_hip_shift.h")
    assert names == ["gten_hip_kv_shift"] == sorted(api.SHIFT_SYMBOLS)
    for name in names:
        assert hasattr(api.lib, name), f"{name} declared in include/gten_hip_shift.h but not exported"
    names = declared("gten_host_shift.h")
    assert len(names) == 13 and names == sorted(h.SHIFT_SYMBOLS)
    for name in names:
        assert hasattr(h.lib, name), f"{name} declared in include/gten_host_shift.h but not exported"
    # the two headers whose symbol lists tests/test_abi_loads.py pins did not grow by them
    for header in ("gten_hip.h", "gten_host.h"):
        assert "shift" not in open(os.path.join(ROOT, "include", header)).read()
    assert pkg.hipabi.GtenHip.SHIFT_ITEM.itemsize == 32             # gten_hip_kv_shift_item
    # host/capi.cpp and the headers it instantiates go on linking against the stand-in of include/gten_hip.h alone: the one
    # translation unit of the library that names the device entry point is host/capi_shift.cpp, through host/generate_shift.h
    hostdir = os.path.join(ROOT, "tinyllama.cpp_amd", "host")
    for f in sorted(os.listdir(hostdir)):
        if f.endswith((".h", ".cpp")) and f not in ("capi_shift.cpp", "generate_shift.h", "tinyllama_cli.cpp"):
            text = open(os.path.join(hostdir, f)).read()
            assert "gten_hip_kv_shift" not in text and '#include "generate_shift.h"' not in text and "gten_hip_shift.h" not in text, f


def test_reference_swaps_are_byte_moves():
    """shift_ref.swap_halves is its own inverse and moves what the definition says, for every layout"""
    rng = np.random.default_rng(0)
    for dtype, d_head, kv_dim in ((ref.F16, 64, 128), (ref.F16, 32, 64), (ref.Q8, 64, 128), (ref.Q8, 32, 64)):
        rb = kv_dim * 2 if dtype == ref.F16 else kv_dim // 32 * 34
        rows = rng.integers(0, 256, (3, rb), dtype=np.uint8)
        sw = ref.swap_halves(rows, dtype, kv_dim, d_head)
        assert np.array_equal(ref.swap_halves(sw, dtype, kv_dim, d_head), rows)
        assert np.array_equal(np.sort(sw, axis=1), np.sort(rows, axis=1))
        if dtype == ref.F16:
            assert np.array_equal(sw.view(np.uint16)[:, : d_head // 2], rows.view(np.uint16)[:, d_head // 2: d_head])
        elif d_head == 64:
            assert np.array_equal(sw[:, :34], rows[:, 34:68])
        else:
            assert np.array_equal(sw[:, :2], rows[:, :2]) and np.array_equal(sw[:, 2:18], rows[:, 18:34])
