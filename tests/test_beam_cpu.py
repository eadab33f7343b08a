"""not gpu: the host's part of beam search (host/beam_plan.h, include/gten_host_beam.h) -- hand-written cases under
sanitizers, the exported plan functions against tests/beam_ref.py on random trellises, and the new symbols in both libraries."""
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

import beam_ref as ref  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402


def test_beam_plan_under_sanitizers(tmp_path):
    """weights, backtracking through duplicated and crossed parents, finalising with 0, some and B finished and with ties
    (tests/host_beam_plan.cpp), under ASan + UBSan.  The program includes host/beam_plan.h alone, and that header is device-free."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = os.path.join(ROOT, "tests", "host_beam_plan.cpp")
    includes = [line for line in open(src) if line.startswith("#include \"")]
    assert includes == ['#include "../tinyllama.cpp_amd/host/beam_plan.h"\n'], includes
    plan = open(os.path.join(ROOT, "tinyllama.cpp_amd", "host", "beam_plan.h")).read()
    assert "#include \"" not in plan and "gten_hip" not in plan          # device-free: the standard library only
    exe = str(tmp_path / "host_beam_plan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           src, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:protect_shadow_gap=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    assert "host_beam_plan ok" in r.stdout


def host():
    pkg = load_package()
    pkg.build.build_all()
    return pkg.hostabi.GtenHost()


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def test_weights_agree_with_the_restatement():
    h = host()
    for max_new in (1, 2, 7, 64):
        for lp in (0.0, 0.5, 0.7, 1.0, 1.3, 2.0):
            got, want = h.beam_weights(max_new, lp), ref.weights(max_new, lp)
            assert got.shape == want.shape and (bits(got) == bits(want)).all(), (max_new, lp)
            assert got[0] == 0.0 and got[1] == 1.0


def random_group(r, B, rounds, n_fin, done):
    """a random trellis of `rounds` rounds and a state with n_fin finished records (finals drawn from a few values: ties)"""
    parent = np.zeros((rounds, 8), np.int32)
    ids = np.zeros((rounds, 8), np.int32)
    parent[1:, :B] = r.integers(0, B, (rounds - 1, B))
    ids[:, :B] = r.integers(0, 512, (rounds, B))
    st = ref.new_state()
    st["t"] = rounds
    grid = np.array([-0.5, -1.0, -1.5, -0.0, 0.0], np.float32)
    st["cum"][:B] = np.where(r.random(B) < 0.5, r.choice(grid, B), -r.random(B).astype(np.float32) * 9)
    for s in range(n_fin):
        t = int(r.integers(1, rounds + 1))
        st["fin_t"][s], st["fin_beam"][s] = t, r.integers(0, 1 if t <= 2 else B)
        st["fin_cum"][s] = -np.float32(r.random()) * 9
        st["fin_final"][s] = r.choice(grid) if r.random() < 0.5 else st["fin_cum"][s] / np.float32(t)
    st["n_fin"], st["done"] = n_fin, done
    return st, parent, ids


def test_plan_functions_agree_with_the_restatement_on_random_trellises():
    h = host()
    r = np.random.default_rng(20)
    n = 0
    for B in (1, 2, 3, 5, 8):
        for rounds in (1, 2, 6, 17):
            w = ref.weights(rounds, 0.8)
            for n_fin in sorted({0, B // 2, B}):
                st, parent, ids = random_group(r, B, rounds, n_fin, 1 if n_fin == B else 0)
                for t in range(rounds + 1):
                    for b in range(B):
                        assert h.beam_backtrack(parent, ids, t, b).tolist() == ref.backtrack(parent, ids, t, b)
                got = h.beam_finalize(st, parent, ids, B, w, rounds)
                want = ref.finalize(st, parent, ids, B, w)
                assert len(got) == len(want) == B
                for (gi, gf, gc, ge), (wi, wf, wc, we) in zip(got, want):
                    assert gi.tolist() == wi and bits(gf) == bits(wf) and bits(gc) == bits(wc) and ge == we, (B, rounds, n_fin)
                n += 1
    assert n == 4 * (2 + 3 + 3 + 3 + 3)
    # outside the trellis
    st, parent, ids = random_group(r, 3, 4, 0, 0)
    assert h.beam_backtrack(parent, ids, 5, 0) is None and h.beam_backtrack(parent, ids, 2, 8) is None
    parent[2, 1] = 11
    assert h.beam_backtrack(parent, ids, 3, 1) is None


def declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gten_(?:hip|host)_[a-z0-9_]+)\s*\(", text)))


def test_both_libraries_export_the_new_names():
    pkg = load_package()
    pkg.build.build_all()
    api, h = pkg.hipabi.GtenHip(), pkg.hostabi.GtenHost()
    names = declared("gten_hip_beam.h")
    assert len(names) == 8 and sorted(api.BEAM_SYMBOLS) == names
    for name in names:
        assert hasattr(api.lib, name), name
    names = declared("gten_host_beam.h")
    assert len(names) == 4 and sorted(h.BEAM_SYMBOLS) == names
    for name in names:
        assert hasattr(h.lib, name), name
    # capi.cpp and what it includes still know nothing of the beam headers (it links against the unchanged tests/hip_stub.cpp)
    seen, todo = set(), [os.path.join(ROOT, "tinyllama.cpp_amd", "host", "capi.cpp")]
    while todo:
        path = todo.pop()
        if path in seen or not os.path.exists(path):
            continue
        seen.add(path)
        text = open(path).read()
        assert "gten_hip_beam" not in text and "beam_search.h" not in text, path
        for inc in re.findall(r'#include "([^"]+)"', text):
            for base in (os.path.dirname(path), os.path.join(ROOT, "tinyllama.cpp_amd"), os.path.join(ROOT, "include")):
                todo.append(os.path.normpath(os.path.join(base, inc)))
