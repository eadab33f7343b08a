"""not gpu: the device-free side of calibrated Q4 loading: the two new headers against their CALIB_SYMBOLS lists
and the exports, disjoint from every other list and header; tests/calib_ref.py's search on a hand case whose winners are known."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from __graft_entry__ import load_package  # noqa: E402
from calib_ref import search_q4, unpack_stream  # noqa: E402
from test_abi_loads import declared_symbols  # noqa: E402


@pytest.mark.parametrize("side, header", [("hipabi.GtenHip", "gten_hip_calib.h"), ("hostabi.GtenHost", "gten_host_calib.h")])
def test_calib_header_is_its_list_exported_and_disjoint(side, header):
    pkg = load_package()
    pkg.build.build_all()
    mod, cls = side.split(".")
    api = getattr(getattr(pkg, mod), cls)()
    names = declared_symbols(header)
    assert names and sorted(api.CALIB_SYMBOLS) == names
    for name in names:
        assert hasattr(api.lib, name), name
        assert name.startswith(("gten_hip_calib_", "gten_host_calib_")) or name == "gten_hip_quantize_weight_search"
    for attr in dir(api):
        if attr.endswith("SYMBOLS") and attr != "CALIB_SYMBOLS":
            assert not set(names) & set(getattr(api, attr)), attr
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != header:
            assert not set(names) & set(declared_symbols(other)), other


def test_reference_search_on_a_hand_case():
    """one row of four blocks, importance 1 except over block 3, where only element 1 counts:
    0  all zero: kept, delta 0
    1  0.5 * (j % 15 - 7): candidate 0 is exact (delta 0.5, err 0), nothing is strictly better
    2  8, then 31 x 1: candidate 0 has delta 8/7 and leaves 0.14 on each 1; the quants (7, 1, ...) first appear at c = 4
       (8 * 6.625 / 8 rounds to 7), give delta 87/80 and win; every later c has the same quants and only ties
    3  7, 0.5, zeros: candidate 0 rounds 0.5 / 1 to 0 (err 0.25); below c = 8 the one weighted quant is 0 (B = 0, invalid); c = 8
       (is > 1) makes it 1, delta = 0.5 / 1, err 0"""
    x = np.zeros((1, 128), np.float32)
    x[0, 32:64] = 0.5 * (np.arange(32) % 15 - 7)
    x[0, 64:96] = 1.0
    x[0, 64] = 8.0
    x[0, 96:98] = (7.0, 0.5)
    imp = np.ones(128, np.float32)
    imp[96:] = 0
    imp[97] = 1
    stream, choice = search_q4(x, imp, "f32", with_choice=True)
    d, q = unpack_stream(stream, 1, 4)
    assert choice.tolist() == [[0, 0, 4, 8]]
    assert d[0].tolist() == [0.0, 0.5, float(np.float16(np.float32(87) / np.float32(80))), 0.5]
    assert not q[0, 0].any() and (q[0, 1] == np.arange(32) % 15 - 7).all()
    assert q[0, 2].tolist() == [7.0] + [1.0] * 31 and q[0, 3].tolist() == [7.0, 1.0] + [0.0] * 30
    plain, choice = search_q4(x, None, "f32", with_choice=True)                      # every weight 1: block 3 now pays for the 7 too
    assert choice[0, :3].tolist() == [0, 0, 4] and (plain[:, :54] == stream[:, :54]).all()
