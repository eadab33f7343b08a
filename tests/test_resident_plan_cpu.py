"""not gpu: which W.x launches of a single-sequence decode step keep their weights in the memory-side cache (host/resident_plan.h,
DESIGN.md §3.2) -- tests/host_resident_plan.cpp plain and under sanitizers, the exported plan against a restatement in Python,
and the new symbols in both libraries.

On TinyLlama's launch list in q4, q8 and f16 and on a two-layer toy list: budget 0 and a budget below the smallest launch give an
empty plan, budget = everything a full one; 192 MiB in q4 gives exactly 22 o + 22 q|k|v + 13 down launches; the plan is monotone in
the budget; the byte sum never exceeds the budget; with equal sizes the earlier launch wins.

The byte sum at 192 MiB: 22 x 2 359 296 + 22 x 2 949 120 + 13 x 6 488 064 = 201 129 984 B -- the per-launch bytes are the packed
layout's (rows x cols / 32 x 18), asserted one by one.  (The figure first written down for this sum, 201 063 424, does not add up
from those three products; the launches it names are the ones asserted here.)"""
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

from __graft_entry__ import load_package  # noqa: E402

SRC = os.path.join(ROOT, "tests", "host_resident_plan.cpp")
PLAN = os.path.join(ROOT, "tinyllama.cpp_amd", "host", "resident_plan.h")
TINYLLAMA = dict(n_layers=22, n_embd=2048, n_ffn=5632, kv_width=256, n_vocab=32003)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_resident_plan_program(tmp_path, sanitize):
    """the stand-alone program (its own main), which includes host/resident_plan.h alone; that header is device-free"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    includes = [line for line in open(SRC) if line.startswith("#include \"")]
    assert includes == ['#include "../tinyllama.cpp_amd/host/resident_plan.h"\n'], includes
    plan = open(PLAN).read()
    assert "#include \"" not in plan and "gten_hip" not in plan and "hip/" not in plan       # the standard library only
    exe = str(tmp_path / "host_resident_plan")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else []
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + flags + [SRC, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:protect_shadow_gap=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-4000:])
    assert "host_resident_plan ok" in r.stdout


def host():
    pkg = load_package()
    pkg.build.build_all()
    return pkg.hostabi.GtenHost()


def restated(each, budget):
    """the rule in Python: ascending weight bytes, ties in step order, whole launches while the sum fits, the first misfit ends it"""
    res, total = np.zeros(len(each), np.uint8), 0
    for i in sorted(range(len(each)), key=lambda i: (int(each[i]), i)):
        if total + int(each[i]) > budget:
            break
        res[i], total = 1, total + int(each[i])
    return res, total


def test_exported_plan_agrees_with_the_restatement():
    h = host()
    shapes = [TINYLLAMA, dict(n_layers=2, n_embd=256, n_ffn=512, kv_width=128, n_vocab=512), dict(n_layers=2, n_embd=512, n_ffn=512, kv_width=128, n_vocab=512),
              dict(n_layers=1, n_embd=64, n_ffn=96, kv_width=32, n_vocab=70)]
    n = 0
    for name, block in sorted(h.RESIDENT_BLOCK_BYTES.items()):
        for sh in shapes:
            E, F, KV, V, L = sh["n_embd"], sh["n_ffn"], sh["kv_width"], sh["n_vocab"], sh["n_layers"]
            _, each, _, _ = h.resident_plan(budget=0, block_bytes=block, **sh)
            want_each = []
            for _l in range(L):
                want_each += [(E + 2 * KV) * (E // 32) * block, E * (E // 32) * block, 2 * F * (E // 32) * block, E * (F // 32) * block]
            want_each.append(V * (E // 32) * block)
            assert each.tolist() == want_each, (name, sh)
            total = int(each.sum())
            budgets = sorted({0, 1, int(each.min()) - 1, int(each.min()), total // 7, total // 3, total // 2, total - 1, total, total + 5} |
                             {int(c) for c in np.cumsum(np.sort(each))} | {int(c) - 1 for c in np.cumsum(np.sort(each))})
            prev = np.zeros(len(each), np.uint8)
            for b in budgets:
                res, _, launches, got = h.resident_plan(budget=b, block_bytes=block, **sh)
                want_res, want_total = restated(each, b)
                assert res.tolist() == want_res.tolist() and got == want_total and launches == int(want_res.sum()), (name, sh, b)
                assert got <= b and (res >= prev).all(), (name, sh, b)
                prev = res
                n += 1
            assert prev.all()
    assert n > 3 * 4 * 10
    # TinyLlama in q4 at 192 MiB: all of o, all of q|k|v, 13 layers of down
    res, each, launches, got = h.resident_plan(budget=192 << 20, block_bytes=18, **TINYLLAMA)
    assert launches == 57 and res[1::4].sum() == 22 and res[0:88:4].sum() == 22 and res[3::4].tolist() == [1] * 13 + [0] * 9
    assert res[2::4].sum() == 0 and res[88] == 0
    assert got == 22 * 2359296 + 22 * 2949120 + 13 * 6488064 == 201129984
    with pytest.raises(Exception):
        h.resident_plan(budget=0, block_bytes=18, n_layers=1, n_embd=100, n_ffn=64, kv_width=32, n_vocab=10)


def declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gten_(?:hip|host)_[a-z0-9_]+)\s*\(", text)))


def test_both_libraries_export_the_new_names():
    pkg = load_package()
    pkg.build.build_all()
    api, h = pkg.hipabi.GtenHip(), pkg.hostabi.GtenHost()
    names = declared("gten_hip_ab.h")
    assert len(names) == 6 and sorted(api.AB_SYMBOLS) == names
    for name in names:
        assert hasattr(api.lib, name), name
    names = declared("gten_host_resident.h")
    assert len(names) == 3 and sorted(h.RESIDENT_SYMBOLS) == names
    for name in names:
        assert hasattr(h.lib, name), name
    # a negative budget is an error and leaves the setting alone
    before = api.weight_resident_bytes()
    assert before >= 0
    with pytest.raises(Exception):
        api.set_weight_resident_mb(-1)
    with pytest.raises(Exception):
        api.set_weight_resident_bytes(-1)
    assert api.weight_resident_bytes() == before
    # the one host unit that names the device's A/B header is host/capi_resident.cpp (host/capi.cpp goes on linking against the
    # stand-in of include/gten_hip.h alone)
    hostdir = os.path.join(ROOT, "tinyllama.cpp_amd", "host")
    for f in sorted(os.listdir(hostdir)):
        if f.endswith((".h", ".cpp")) and f != "capi_resident.cpp":
            text = open(os.path.join(hostdir, f), errors="replace").read()
            assert "gten_hip_ab.h" not in text and "gten_hip_set_weight_resident" not in text and "gten_hip_decoder_resident" not in text, f
