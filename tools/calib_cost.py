"""What calibrated Q4 loading costs and gains -> profiles/calib_cost.json.  Report only: nothing here is a threshold.

  search   k_quant_search (f16 source, random positive importance) on 5632 x 2048 and 2048 x 2048 beside k_quant_pack on the same
           source, alternating call by call: the time between the library's profiler events around the launch (median, least and
           largest of --reps calls after 3 warm-up calls)
  energy   gten_hip_calib_col_energy (both launches) on 4096 x 2048 Q8 and f16 rows, the same way
  quality  SYNTHETIC Gaussian weights (no trained checkpoint is used): a 4-layer model of width 512 / 1024 in f16 mode and as q4 loaded
           plain, through the search without importance, and through the search with importance collected on 8 texts of 64 ids:
           the rms of the logit difference to the f16-mode model over the last rows of 16 held-out texts

    python tools/calib_cost.py [--reps 20] [--out profiles/calib_cost.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402


def timed(hip, family, launches, call):
    before = hip.prof_read().get(family, (0, 0.0))
    hip._check(call())
    after = hip.prof_read()[family]
    assert after[0] == before[0] + launches
    return (after[1] - before[1]) * 1e3


def stat(t):
    return {"median": round(statistics.median(t), 2), "min": round(min(t), 2), "max": round(max(t), 2)}


def search_cost(hip, rows, cols, reps):
    rng = np.random.default_rng(rows)
    src = hip.upload((rng.standard_normal((rows, cols)) * 0.05).astype(np.float16))
    imp, out = hip.upload(rng.uniform(0.25, 4.0, cols).astype(np.float32)), hip.alloc(rows * hip.row_bytes(4, cols))
    plain, search = [], []
    for i in range(reps + 3):
        p = timed(hip, "pack_weight", 1, lambda: hip.quantize_weight_rc(src, "f16", rows, cols, 4, out))
        s = timed(hip, "pack_weight", 1, lambda: hip.quantize_weight_search_rc(src, "f16", rows, cols, imp, out))
        if i >= 3:
            plain.append(p)
            search.append(s)
    for buf in (src, imp, out):
        buf.free()
    return {"rows": rows, "cols": cols, "src": "f16", "reps": reps, "k_quant_pack_us": stat(plain), "k_quant_search_us": stat(search)}


def energy_cost(hip, adtype, n_rows, cols, reps):
    rows = hip.alloc(n_rows * hip.row_bytes(adtype, cols))
    rows.zero(0x11)                                                 # (finite in both storage forms)
    acc = hip.upload(np.zeros(cols, np.float64))
    t = [timed(hip, "elementwise", 2, lambda: hip.calib_col_energy_rc(rows, adtype, n_rows, cols, acc)) for _ in range(reps + 3)][3:]
    rows.free()
    acc.free()
    return {"adtype": {1: "f16", 3: "q8"}[adtype], "rows": n_rows, "cols": cols, "reps": reps, "col_energy_us": stat(t)}


def quality(pkg, host):
    rng = np.random.default_rng(5)

    def model(wd, ad):
        cfg = host.default_config(wd, ad)
        cfg.n_vocab, cfg.max_ctx, cfg.n_embd, cfg.n_ffn, cfg.n_layers, cfg.n_heads, cfg.n_kv_heads = 2048, 128, 512, 1024, 4, 8, 4
        return host.model(cfg), cfg
    f16, cfg = model(1, 1)
    weights = [(rng.standard_normal((r, c)) * (c ** -0.5 if r > 1 else 1.0)).astype(np.float16).reshape((r, c) if r > 1 else (c,))
               for r, c, _ in cfg.weight_shapes()]
    calib = [rng.integers(0, cfg.n_vocab, 64).astype(np.int32) for _ in range(8)]
    held = [rng.integers(0, cfg.n_vocab, 64).astype(np.int32) for _ in range(16)]
    for i, w in enumerate(weights):
        f16.set_weight_from(i, w, "f16")
    want = np.stack([f16.logits(t, 0) for t in held])
    f16.close()
    def q4_model(importance_of):
        m, _ = model(4, 3)
        for i, w in enumerate(weights):
            block = 0 < i < len(weights) - 2 and (i - 1) % 9 < 7
            m.set_weight_from(i, w, "f16", importance=importance_of(i, w) if block else None)
        return m
    plain = q4_model(lambda i, w: None)
    collected = plain.collect_importance(calib)                      # collected on the plain q4 model
    models = {"plain": plain, "search_no_importance": q4_model(lambda i, w: np.ones(w.shape[1], np.float32)),
              "search_collected_importance": q4_model(lambda i, w: collected[i])}
    res = {}
    for name, m in models.items():
        got = np.stack([m.logits(t, 0) for t in held])
        m.close()
        res[name] = round(float(np.sqrt(np.mean((got - want) ** 2))), 5)
    res["logit_rms_of_the_f16_model"] = round(float(np.sqrt(np.mean(want ** 2))), 5)
    return {"weights": "synthetic Gaussian, 4 layers, 512 / 1024, vocabulary 2048", "rms_of_logit_difference_to_f16_mode": res}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calib_cost.json"))
    a = ap.parse_args()
    pkg = load_package()
    hip = pkg.hipabi.load()
    if hip.device_count() < 1:
        raise SystemExit("no GPU visible: nothing here can be measured without one")
    hip.init(0)
    hip.prof_enable(True)
    res = {"search": [search_cost(hip, r, 2048, a.reps) for r in (5632, 2048)],
           "energy": [energy_cost(hip, dt, 4096, 2048, a.reps) for dt in (3, 1)]}
    hip.prof_enable(False)
    res["quality"] = quality(pkg, pkg.load_host())
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
