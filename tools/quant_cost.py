"""What quantising on the device costs -> profiles/quant_cost.json.  Report only: nothing here is a threshold.

  kernel   k_quant_pack on an f16 source, q4 and q8, on a 5632 x 2048 matrix and on the lm_head (32003 x 2048): the time between
           the library's profiler events around the launch (median of --reps calls after a warm-up) and the bytes the kernel
           must move (source read once + packed weight written once) over that time
  load     (--full) the full-size model, file to first logits: load_gten of the q4 file the converter wrote, load_gten_f16 of
           the f16 file, and the NumPy converter's own run (f16 records -> q4 file) beside them, for scale; host wall clock
           around work that ends in a device-to-host copy of the logits

    python tools/quant_cost.py [--full] [--reps 20] [--out profiles/quant_cost.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

CODES = {"q8": 3, "q4": 4}


def kernel_cost(hip, rows, cols, dst, reps):
    w = (np.random.default_rng(rows).standard_normal((rows, cols)) * 0.05).astype(np.float16)
    src, out = hip.upload(w), hip.alloc(rows * hip.row_bytes(CODES[dst], cols))
    times = []
    for i in range(reps + 3):
        before = hip.prof_read().get("pack_weight", (0, 0.0))
        hip._check(hip.quantize_weight_rc(src, "f16", rows, cols, CODES[dst], out))
        after = hip.prof_read()["pack_weight"]
        assert after[0] == before[0] + 1
        if i >= 3:
            times.append((after[1] - before[1]) * 1e3)
    src.free()
    out.free()
    moved = w.nbytes + rows * hip.row_bytes(CODES[dst], cols)
    us = statistics.median(times)
    return {"rows": rows, "cols": cols, "src": "f16", "dst": dst, "kernel_us_median": round(us, 2), "kernel_us_min": round(min(times), 2),
            "kernel_us_max": round(max(times), 2), "bytes_moved": moved, "achieved_GB_per_s": round(moved / us / 1e3, 1), "reps": reps}


def first_logits(host, cfg, load):
    t0 = time.perf_counter()
    m = host.model(cfg)
    load(m)
    lg = m.logits(np.array([1, 5, 9], np.int32), 0)
    dt = time.perf_counter() - t0
    m.close()
    return dt, lg


def load_cost(pkg, host, tmp):
    import importlib
    convert = importlib.import_module(pkg.__name__ + ".convert")
    cfg16, cfg4 = host.default_config(1, 1), host.default_config(4, 3)
    f16, q4 = os.path.join(tmp, "m.f16.gten"), os.path.join(tmp, "m.q4.gten")
    host.write_gten(cfg16, 7, f16)
    shapes = iter(cfg16.weight_shapes())
    t0 = time.perf_counter()
    with open(f16, "rb") as f:
        f.seek(8)

        def record(name):
            rows, cols, _ = next(shapes)
            f.seek(2 * (4 + len(name.encode())) + 4, 1)
            return np.fromfile(f, np.float16, rows * cols).astype(np.float32).reshape(rows, cols), "f16"
        convert.write_gten(q4, record, cfg16.n_layers, "q4")
    numpy_s = time.perf_counter() - t0
    out = {"numpy_convert_f16_to_q4_file_s": round(numpy_s, 2), "f16_file_bytes": os.path.getsize(f16), "q4_file_bytes": os.path.getsize(q4), "runs": []}
    for rep in range(3):                                   # alternating; the first pair also pays the page cache and code objects
        a, la = first_logits(host, cfg4, lambda m: m.load_gten(q4))
        b, lb = first_logits(host, cfg4, lambda m: m.load_gten_f16(f16))
        assert la.tobytes() == lb.tobytes()
        out["runs"].append({"load_gten_q4_file_s": round(a, 3), "load_gten_f16_s": round(b, 3)})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quant_cost.json"))
    a = ap.parse_args()
    pkg = load_package()
    hip = pkg.hipabi.load()
    if hip.device_count() < 1:
        raise SystemExit("no GPU visible: nothing here can be measured without one")
    hip.init(0)
    hip.prof_enable(True)
    res = {"kernel": [kernel_cost(hip, r, 2048, d, a.reps) for r in (5632, 32003) for d in ("q4", "q8")]}
    hip.prof_enable(False)
    if a.full:
        with tempfile.TemporaryDirectory() as tmp:
            res["load"] = load_cost(pkg, pkg.load_host(), tmp)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
