"""What loading GPTQ / AWQ 4-bit tensors on the device costs -> profiles/w4_cost.json.  Report only: nothing here is a threshold.

  kernel   k_quant_w4 into q4 and f16 for GPTQ, GPTQ with a non-trivial g_idx and AWQ on 2048 x 2048 and 5632 x 2048 (N x K), group 128:
           the time between the library's profiler events around the launch (median, least and largest of --reps calls after a
           warm-up), the bytes the kernel must move (the four source tensors read once + the destination written once) over that
           time; beside it gten_hip_quantize_weight_gguf for Q4_0 on the same shapes from the same run -- a comparable launch, not a
           target.  The launches repeat on one buffer, which may sit in the last-level cache: these are not cold-HBM figures.
  load     (--full) the full-size model from a synthetic GPTQ and AWQ safetensors file (random words, group 128, f16 embed_tokens /
           lm_head / norms), file to first logits through load_quantized; beside it the host's way for the seven linears of BLOCK 0
           only: tests/w4_ref.py's NumPy dequantisation, then set_weight_from(..., "f16") -- host wall clock, its two parts apart

    python tools/w4_cost.py [--full] [--reps 20] [--out profiles/w4_cost.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gguf_ref  # noqa: E402
import w4_ref  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

CASES = [("gptq", False), ("gptq", True), ("awq", False)]


def timed(hip, reps, call):
    times = []
    for i in range(reps + 3):
        before = hip.prof_read().get("pack_weight", (0, 0.0))
        hip._check(call())
        after = hip.prof_read()["pack_weight"]
        assert after[0] == before[0] + 1
        if i >= 3:
            times.append((after[1] - before[1]) * 1e3)
    return {"kernel_us_median": round(statistics.median(times), 2), "kernel_us_min": round(min(times), 2), "kernel_us_max": round(max(times), 2), "reps": reps}


def kernel_cost(hip, layout, act, n, k, dst, reps):
    src = w4_ref.random_source(layout, n, k, 128, np.random.default_rng(n + k), act)
    bufs = [None if a is None else hip.upload(np.ascontiguousarray(a).view(np.uint8).reshape(-1)) for a in src]
    out = hip.alloc(n * hip.row_bytes(dst, k))
    res = timed(hip, reps, lambda: hip.quantize_weight_w4_rc(*bufs, layout, 0, n, k, 128, dst, out))
    moved = sum(a.nbytes for a in src if a is not None) + n * hip.row_bytes(dst, k)
    for b in bufs + [out]:
        if b is not None:
            b.free()
    return dict({"layout": layout, "g_idx": act, "rows": n, "cols": k, "group_size": 128, "dst": {4: "q4", 1: "f16"}[dst], "bytes_moved": moved,
                 "achieved_GB_per_s": round(moved / res["kernel_us_median"] / 1e3, 1)}, **res)


def gguf_cost(hip, n, k, reps):
    stream = gguf_ref.random_stream(2, n, k, np.random.default_rng(2))
    src, out = hip.upload(stream), hip.alloc(n * hip.row_bytes(4, k))
    res = timed(hip, reps, lambda: hip.quantize_weight_gguf_rc(src, 2, n, k, 4, out))
    src.free()
    out.free()
    moved = stream.nbytes + n * hip.row_bytes(4, k)
    return dict({"format": "Q4_0 (gten_hip_quantize_weight_gguf)", "rows": n, "cols": k, "dst": "q4", "bytes_moved": moved,
                 "achieved_GB_per_s": round(moved / res["kernel_us_median"] / 1e3, 1)}, **res)


def load_cost(pkg, host, tmp, layout, act):
    from safetensors.numpy import save_file
    convert = importlib.import_module(pkg.__name__ + ".convert")
    cfg = host.default_config(4, 3)
    rng = np.random.default_rng(5)
    names = [n for n, _ in convert.tensor_names(cfg.n_layers)]
    tensors, block0 = {}, []
    for idx, (name, (rows, cols, dt)) in enumerate(zip(names, cfg.weight_shapes())):
        if dt == 1 or "layers" not in name:
            tensors[name] = np.ones(cols, np.float16) if dt == 1 else (rng.standard_normal((rows, cols)) * 0.02).astype(np.float16)
            continue
        src = w4_ref.random_source(layout, rows, cols, 128, rng, act, scale_max=0.005)
        tensors.update({f"{name[:-7]}.{part}": a for part, a in zip(("qweight", "qzeros", "scales", "g_idx"), src) if a is not None})
        if name.startswith("model.layers.0."):
            block0.append((idx, src))
    d = os.path.join(tmp, layout + ("_act" if act else ""))
    os.makedirs(d)
    save_file(tensors, os.path.join(d, "model.safetensors"))
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump({"quantization_config": {"quant_method": layout, "bits": 4, "group_size": 128, "desc_act": act, "version": "gemm", "checkpoint_format": "gptq_v2"}}, f)
    out = {"layout": layout, "g_idx": act, "file_bytes": os.path.getsize(os.path.join(d, "model.safetensors")),
           "f32_bytes_of_the_same_tensors": sum(4 * r * c for r, c, _ in cfg.weight_shapes()), "runs": []}
    for rep in range(3):                                   # the first run also pays the page cache and the code objects
        t0 = time.perf_counter()
        m = host.model(cfg)
        m.load_quantized(d)
        lg = m.logits(np.array([1, 5, 9], np.int32), 0)
        out["runs"].append({"load_quantized_to_first_logits_s": round(time.perf_counter() - t0, 3), "logits_finite": bool(np.isfinite(lg).all())})
        m.close()
    m = host.model(cfg)
    a = b = 0.0
    for idx, src in block0:
        t0 = time.perf_counter()
        x = w4_ref.dequant(layout, *src, 0, 128).astype(np.float16)
        t1 = time.perf_counter()
        m.set_weight_from(idx, x, "f16")
        a, b = a + t1 - t0, b + time.perf_counter() - t1
    m.quant_release()
    m.close()
    out["host_way_block0_only"] = {"numpy_dequant_s": round(a, 3), "upload_f16_and_quantise_s": round(b, 3), "blocks_in_the_model": cfg.n_layers}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "w4_cost.json"))
    a = ap.parse_args()
    pkg = load_package()
    hip = pkg.hipabi.load()
    if hip.device_count() < 1:
        raise SystemExit("no GPU visible: nothing here can be measured without one")
    hip.init(0)
    hip.prof_enable(True)
    res = {"kernel": [], "gguf_q4_0": [], "caveat": "repeated launches on one buffer: the source may sit in the last-level cache; random words, no trained checkpoint"}
    for n, k in ((2048, 2048), (5632, 2048)):
        res["gguf_q4_0"].append(gguf_cost(hip, n, k, a.reps))
        res["kernel"] += [kernel_cost(hip, layout, act, n, k, dst, a.reps) for layout, act in CASES for dst in (4, 1)]
    hip.prof_enable(False)
    if a.full:
        with tempfile.TemporaryDirectory() as tmp:
            host = pkg.load_host()
            res["load"] = [load_cost(pkg, host, tmp, layout, act) for layout, act in (("gptq", False), ("awq", False))]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
