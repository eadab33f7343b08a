"""What loading GGUF tensors on the device costs -> profiles/gguf_cost.json.  Report only: nothing here is a threshold.

  kernel   k_quant_gguf into q4 for each of the six formats on a 32003 x 2048 and a 2048 x 5632 tensor: the time between the
           library's profiler events around the launch (median of --reps calls after a warm-up), the bytes the kernel must move
           (block stream read once + packed weight written once) over that time, and the stream's bytes beside the f32 matrix's
  load     (--full) the full-size model from a synthetic GGUF file (linears and token_embd Q4_K, output Q6_K, norms F32, random
           block bytes), file to first logits through load_gguf; beside it the host's way for token_embd, the tensors of block 0
           and output: tests/gguf_ref.py's dequant to f32, then set_weight_from(..., "f32") -- its two parts timed apart, and
           block 0's sum times the number of blocks as a PROJECTION of the whole model's; host wall clock

    python tools/gguf_cost.py [--full] [--reps 20] [--out profiles/gguf_cost.json]
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
from __graft_entry__ import load_package  # noqa: E402


def kernel_cost(hip, code, rows, cols, reps):
    stream = gguf_ref.random_stream(code, rows, cols, np.random.default_rng(code))
    src, out = hip.upload(stream), hip.alloc(rows * hip.row_bytes(4, cols))
    times = []
    for i in range(reps + 3):
        before = hip.prof_read().get("pack_weight", (0, 0.0))
        hip._check(hip.quantize_weight_gguf_rc(src, code, rows, cols, 4, out))
        after = hip.prof_read()["pack_weight"]
        assert after[0] == before[0] + 1
        if i >= 3:
            times.append((after[1] - before[1]) * 1e3)
    src.free()
    out.free()
    moved = stream.nbytes + rows * hip.row_bytes(4, cols)
    us = statistics.median(times)
    return {"format": gguf_ref.FORMATS[code][0], "rows": rows, "cols": cols, "dst": "q4", "kernel_us_median": round(us, 2), "kernel_us_min": round(min(times), 2),
            "kernel_us_max": round(max(times), 2), "stream_bytes": stream.nbytes, "f32_bytes": rows * cols * 4, "bytes_moved": moved,
            "achieved_GB_per_s": round(moved / us / 1e3, 1), "reps": reps}


def load_cost(pkg, host, tmp):
    convert = importlib.import_module(pkg.__name__ + ".convert")
    cfg = host.default_config(4, 3)
    rng = np.random.default_rng(5)
    names = [n for n, _ in convert.tensor_names(cfg.n_layers)]
    back = {convert._gguf_hf_name(g): g for g in ["token_embd.weight", "output_norm.weight", "output.weight"] +
            [f"blk.{i}.{k}.weight" for i in range(cfg.n_layers) for k in convert._GGUF_BLOCK]}
    tensors = []
    for name, (rows, cols, dt) in zip(names, cfg.weight_shapes()):
        if dt == 1:
            tensors.append((back[name], 0, (cols,), np.ones(cols, np.float32).tobytes()))
        else:
            code = 14 if name == "lm_head.weight" else 12
            tensors.append((back[name], code, (rows, cols), gguf_ref.random_stream(code, rows, cols, rng, d_max=2e-4)))
    path = os.path.join(tmp, "m.gguf")
    gguf_ref.write_gguf(path, tensors, {"llama.block_count": cfg.n_layers, "llama.attention.head_count": cfg.n_heads,
                                        "llama.attention.head_count_kv": cfg.n_kv_heads})
    out = {"gguf_file_bytes": os.path.getsize(path), "f32_bytes_of_the_same_tensors": sum(4 * r * c for r, c, _ in cfg.weight_shapes()), "runs": []}
    for rep in range(3):                                   # the first run also pays the page cache and the code objects
        t0 = time.perf_counter()
        m = host.model(cfg)
        m.load_gguf(path)
        lg = m.logits(np.array([1, 5, 9], np.int32), 0)
        out["runs"].append({"load_gguf_to_first_logits_s": round(time.perf_counter() - t0, 3), "logits_finite": bool(np.isfinite(lg).all())})
        m.close()
    m = host.model(cfg)
    part = {}
    for idx in [0] + list(range(1, 10)) + [len(names) - 1]:
        _, code, shape, raw = tensors[idx]
        t0 = time.perf_counter()
        x = gguf_ref.dequant(raw, code, *shape) if code in gguf_ref.FORMATS else np.frombuffer(raw, np.float32)
        t1 = time.perf_counter()
        m.set_weight_from(idx, x, "f32")
        key = "token_embd" if idx == 0 else "output" if idx > 9 else "block0"
        a, b, n = part.get(key, (0.0, 0.0, 0))
        part[key] = (a + t1 - t0, b + time.perf_counter() - t1, n + x.nbytes)
    m.quant_release()
    m.close()
    out["host_way"] = {k: {"numpy_dequant_s": round(a, 3), "upload_f32_and_quantise_s": round(b, 3), "f32_bytes_uploaded": n} for k, (a, b, n) in part.items()}
    L = cfg.n_layers
    out["host_way"]["projection_whole_model_s"] = {"numpy_dequant": round(part["token_embd"][0] + part["output"][0] + L * part["block0"][0], 2),
                                                   "upload_f32_and_quantise": round(part["token_embd"][1] + part["output"][1] + L * part["block0"][1], 2)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gguf_cost.json"))
    a = ap.parse_args()
    pkg = load_package()
    hip = pkg.hipabi.load()
    if hip.device_count() < 1:
        raise SystemExit("no GPU visible: nothing here can be measured without one")
    hip.init(0)
    hip.prof_enable(True)
    res = {"kernel": [kernel_cost(hip, code, r, c, a.reps) for code in sorted(gguf_ref.FORMATS) for r, c in ((32003, 2048), (2048, 5632))]}
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
