"""not gpu: n samples per prompt (include/gten_hip_groups.h, include/gten_host_samples.h).  The two new headers declare exactly the
new names, the libraries export them, the bindings' lists match; GTEN_GROUPS_MAX is 64 beside an unchanged GTEN_PREFIXES_MAX; only
host/capi_samples.cpp names the device entry points; gten_host_samples_rank -- device-free -- agrees with tests/samples_ref.py on
200 seeded cases; and the expansion and the output order are what the restatement says."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from __graft_entry__ import load_package  # noqa: E402
from test_abi_loads import declared_symbols  # noqa: E402
import samples_ref  # noqa: E402

HIP_NAMES = ["gten_hip_decoder_group_set", "gten_hip_decoder_group_share", "gten_hip_decoder_groups_info"]
HOST_NAMES = ["gten_host_batch_group_decode_set", "gten_host_batch_group_decode_share", "gten_host_batch_groups_decode_info",
              "gten_host_batch_samples_info", "gten_host_batch_serve_samples", "gten_host_batch_set_groups_cap", "gten_host_samples_rank",
              "gten_host_samples_rank_records"]


def test_hip_library_exports_the_groups_header():
    pkg = load_package()
    pkg.build.build_hip()
    api = pkg.hipabi.GtenHip()
    names = declared_symbols("gten_hip_groups.h")
    assert names == HIP_NAMES
    for name in names:
        assert hasattr(api.lib, name), f"{name} declared in include/gten_hip_groups.h but not exported"
    assert sorted(api.GROUPS_SYMBOLS) == names, "python binding out of sync with the header"
    for m in ("decoder_group_set", "decoder_group_share", "decoder_groups_info"):
        assert callable(getattr(pkg.hipabi.GtenHip, m)), m
    text = open(os.path.join(ROOT, "include", "gten_hip_groups.h")).read()
    assert re.search(r"#define\s+GTEN_GROUPS_MAX\s+64\b", text) and api.GROUPS_MAX == 64
    text = open(os.path.join(ROOT, "include", "gten_hip_prefixes.h")).read()
    assert re.search(r"#define\s+GTEN_PREFIXES_MAX\s+8\b", text) and api.PREFIXES_MAX == 8


def test_host_library_exports_the_samples_header():
    pkg = load_package()
    pkg.build.build_all()
    host = pkg.hostabi.GtenHost()
    names = declared_symbols("gten_host_samples.h")
    assert names == HOST_NAMES
    for name in names:
        assert hasattr(host.lib, name), f"{name} declared in include/gten_host_samples.h but not exported"
    assert sorted(host.SAMPLES_SYMBOLS) == names
    for m in ("serve_samples", "serve_samples_items", "samples_info", "set_groups_cap", "groups_decode_info"):
        assert callable(getattr(pkg.hostabi.HostBatch, m)), m
    assert callable(pkg.hostabi.GtenHost.samples_rank)
    assert host.GROUPS_MAX == 64


def test_the_other_headers_do_not_grow_and_one_unit_names_the_device_calls():
    pkg = load_package()
    hip, host = pkg.hipabi.GtenHip, pkg.hostabi.GtenHost
    assert not set(hip.GROUPS_SYMBOLS) & set(hip.SYMBOLS + hip.PREFIX_DECODE_SYMBOLS + hip.PREFIXES_SYMBOLS)
    assert not set(host.SAMPLES_SYMBOLS) & set(host.SYMBOLS + host.FSM_SYMBOLS + host.PREFIXES_SYMBOLS)
    pat = re.compile(r"\b(%s)\b" % "|".join(HIP_NAMES + HOST_NAMES))
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h in ("gten_hip_groups.h", "gten_host_samples.h"):
            continue
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
        assert not pat.search(text), h
    # host/capi.cpp and the headers it instantiates reach the group records through hooks only (it links against the test
    # stand-in of include/gten_hip.h alone): the one translation unit that names them is host/capi_samples.cpp
    dev = re.compile(r"\b(%s)\b" % "|".join(HIP_NAMES))
    for base, _, files in os.walk(os.path.join(ROOT, "tinyllama.cpp_amd")):
        if os.path.basename(base) == "csrc":
            continue                                   # (the library that defines them)
        for f in files:
            if not f.endswith((".h", ".cpp")) or f == "capi_samples.cpp":
                continue
            text = re.sub(r"//[^\n]*|/\*.*?\*/", "", open(os.path.join(base, f), errors="replace").read(), flags=re.S)
            assert not dev.search(text), os.path.join(base, f)


def test_rank_agrees_with_the_python_restatement():
    pkg = load_package()
    pkg.build.build_all()
    host = pkg.hostabi.GtenHost()
    cases = samples_ref.rank_cases(200)
    assert len(cases) == 200
    ties = empties = 0
    for rec, n_prompt, n_new in cases:
        sums = samples_ref.record_sums(rec, n_prompt, n_new)
        want = samples_ref.rank(sums, n_new)
        assert host.samples_rank(sums, n_new).tolist() == want, (sums, n_new)
        assert host.samples_rank_records(rec, n_prompt, n_new).tolist() == want, (sums, n_new)
        means = [s / n for s, n in zip(sums, n_new) if n > 0]
        ties += len(set(means)) < len(means)
        empties += 0 in n_new
    assert ties >= 40 and empties >= 20                # (the cases hold ties and samples without new ids)
    # the properties by hand
    assert host.samples_rank([-2.0, -1.0, -3.0], [1, 1, 1]).tolist() == [1, 0, 2]
    assert host.samples_rank([-2.0, -4.0], [1, 4]).tolist() == [1, 0]                  # the MEAN, not the sum
    assert host.samples_rank([-1.0, -2.0, -1.0], [1, 2, 1]).tolist() == [0, 1, 2]      # ties: the lower sample
    assert host.samples_rank([0.0, -5.0, 0.0], [0, 5, 0]).tolist() == [1, 0, 2]        # no new ids: last, by index
    assert host.samples_rank([], []).tolist() == []
    with pytest.raises(ValueError):
        host.samples_rank([0.0], [-1])


def test_expansion_and_output_order():
    n = [1, 3, 2, 5, 1]
    first = samples_ref.first_items(n)
    assert first == [0, 1, 4, 6, 11, 12]
    prompts = ["a", "b", "c", "d", "e"]
    items = samples_ref.expand(prompts, n)
    assert items == ["a", "b", "b", "b", "c", "c", "d", "d", "d", "d", "d", "e"]
    # sample i of prompt j is item first[j] + i; the outputs come back in that order and regroup is the inverse
    for j in range(len(n)):
        for i in range(n[j]):
            assert items[first[j] + i] == prompts[j]
    assert samples_ref.regroup(list(range(12)), n) == [[0], [1, 2, 3], [4, 5], [6, 7, 8, 9, 10], [11]]
    assert samples_ref.regroup(items, n) == [[p] * k for p, k in zip(prompts, n)]
    # the binding expands per-prompt requests the same way
    pkg = load_package()
    assert pkg.hostabi._samples_counts(3, 4).tolist() == [3, 3, 3, 3]
    assert np.repeat(np.asarray([7, 8, 9]), pkg.hostabi._samples_counts([2, 1, 3], 3)).tolist() == samples_ref.expand([7, 8, 9], [2, 1, 3])
    with pytest.raises(AssertionError):
        pkg.hostabi._samples_counts([0, 1], 2)
    with pytest.raises(AssertionError):
        pkg.hostabi._samples_counts(65, 2)
