"""What merging a LoRA adapter while quantising costs -> profiles/lora_cost.json.  Report only: nothing here is a
threshold.

  kernel   k_quant_pack_lora (f16 source, f16 adapter, q4) on 5632 x 2048 and 2048 x 2048 at ranks 8, 16 and 64, beside k_quant_pack
           on the same source: the time between the library's profiler events around the launch (median, least and largest of
           --reps calls after 3 warm-up calls, the two kernels alternating call by call), and the 2 * rank VALU operations per
           element over the difference of the medians
  load     (--full) HostModel.load_checkpoint of a synthetic full-size f16 safetensors checkpoint into a q4 model, without and with
           a rank-16 adapter on all seven linear weights of every block, alternating, three pairs: host wall clock around
           create + load + a 3-id prompt's logits (which ends in a device-to-host copy)

    python tools/lora_cost.py [--full] [--reps 20] [--out profiles/lora_cost.json]
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
from __graft_entry__ import load_package  # noqa: E402


def timed(hip, call):
    before = hip.prof_read().get("pack_weight", (0, 0.0))
    hip._check(call())
    after = hip.prof_read()["pack_weight"]
    assert after[0] == before[0] + 1
    return (after[1] - before[1]) * 1e3


def kernel_cost(hip, rows, cols, rank, reps):
    rng = np.random.default_rng(rows + rank)
    w, a, b = ((rng.standard_normal(s) * 0.05).astype(np.float16) for s in ((rows, cols), (rank, cols), (rows, rank)))
    src, da, db, out = hip.upload(w), hip.upload(a), hip.upload(b), hip.alloc(rows * hip.row_bytes(4, cols))
    plain, lora = [], []
    for i in range(reps + 3):
        p = timed(hip, lambda: hip.quantize_weight_rc(src, "f16", rows, cols, 4, out))
        m = timed(hip, lambda: hip.quantize_weight_lora_rc(src, "f16", rows, cols, da, db, rank, "f16", 2.0, 4, out))
        if i >= 3:
            plain.append(p)
            lora.append(m)
    for buf in (src, da, db, out):
        buf.free()
    stat = lambda t: {"median": round(statistics.median(t), 2), "min": round(min(t), 2), "max": round(max(t), 2)}
    extra = statistics.median(lora) - statistics.median(plain)
    return {"rows": rows, "cols": cols, "rank": rank, "src": "f16", "ab": "f16", "dst": "q4", "reps": reps, "k_quant_pack_us": stat(plain),
            "k_quant_pack_lora_us": stat(lora), "valu_ops": 2 * rank * rows * cols,
            "valu_Tops_per_s_over_the_difference": round(2 * rank * rows * cols / extra / 1e6, 2) if extra > 0 else None}


def load_cost(pkg, host, tmp):
    from safetensors.numpy import save_file
    convert = importlib.import_module(pkg.__name__ + ".convert")
    cfg = host.default_config(4, 3)
    rng = np.random.default_rng(3)
    names = [n for n, _ in convert.tensor_names(cfg.n_layers)]
    tensors, adapters = {}, {}
    for name, (r, c, _) in zip(names, cfg.weight_shapes()):
        tensors[name] = (rng.standard_normal((r, c), np.float32) * (0.05 if r > 1 else 1.0)).astype(np.float16).reshape((r, c) if r > 1 else (c,))
        if "_proj." in name:
            adapters[name] = ((rng.standard_normal((16, c), np.float32) * 0.05).astype(np.float16), (rng.standard_normal((r, 16), np.float32) * 0.05).astype(np.float16))
    path = os.path.join(tmp, "model.safetensors")
    save_file(tensors, path)
    del tensors

    def first_logits(lora):
        t0 = time.perf_counter()
        m = host.model(cfg)
        m.load_checkpoint(path, lora=lora)
        lg = m.logits(np.array([1, 5, 9], np.int32), 0)
        dt = time.perf_counter() - t0
        m.close()
        assert np.isfinite(lg).all()
        return round(dt, 3)

    runs = [{"load_checkpoint_s": first_logits(None), "load_checkpoint_lora_s": first_logits((adapters, 2.0))} for _ in range(3)]
    return {"checkpoint_bytes": os.path.getsize(path), "adapted_weights": len(adapters), "rank": 16, "runs": runs}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lora_cost.json"))
    a = ap.parse_args()
    pkg = load_package()
    hip = pkg.hipabi.load()
    if hip.device_count() < 1:
        raise SystemExit("no GPU visible: nothing here can be measured without one")
    hip.init(0)
    hip.prof_enable(True)
    res = {"kernel": [kernel_cost(hip, r, 2048, k, a.reps) for r in (5632, 2048) for k in (8, 16, 64)]}
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
