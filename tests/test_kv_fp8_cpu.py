"""not gpu: the FP8 K / V shadows' rounding and layout without a device: csrc/gten_kvfp8_math.h in a stand-alone program
under ASan + UBSan (tests/host_kvfp8_math.cpp); the NumPy restatement against a float64 nearest-value search over all 65 536 patterns."""
import os
import subprocess

import numpy as np

import kv_fp8_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shared_header_under_sanitizers(tmp_path):
    src, exe = os.path.join(ROOT, "tests", "host_kvfp8_math.cpp"), str(tmp_path / "host_kvfp8_math")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", src, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "host_kvfp8_math ok" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def test_restatement_is_the_nearest_e4m3_value():
    """float64 search: the 127 finite magnitudes by the format's definition, every f16 pattern to the nearest, a tie to the even code"""
    codes = np.arange(127)
    E, m = codes >> 3, codes & 7
    mags = np.where(E > 0, (8.0 + m) * 2.0 ** (E - 10.0), m * 2.0 ** -9)
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    with np.errstate(invalid="ignore"):
        x = np.abs(h.view(np.float16).astype(np.float64))
        dist = np.abs(np.minimum(x, 1e6)[:, None] - mags[None, :])            # (an infinity is beyond 448 like any large value)
    tied = dist == dist.min(axis=1, keepdims=True)
    even = tied & (codes % 2 == 0)[None, :]
    want = np.where(tied.sum(axis=1) == 2, even.argmax(axis=1), tied.argmax(axis=1)).astype(np.uint8) | ((h >> 15) << 7).astype(np.uint8)
    want[np.isnan(x)] = 0
    got = ref.r8(h)
    assert np.array_equal(got, want) and not ((got & 0x7f) == 0x7f).any()
    back = ref.e8(np.arange(256, dtype=np.uint16).astype(np.uint8))
    finite = (np.arange(256) & 0x7f) != 0x7f
    assert np.array_equal(np.abs(back.view(np.float16).astype(np.float64))[:127], mags) and np.array_equal(back >> 15, np.arange(256) >> 7)
    assert np.array_equal(ref.r8(back)[finite], np.arange(256, dtype=np.uint16).astype(np.uint8)[finite])      # R is idempotent

