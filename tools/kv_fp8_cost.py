#!/usr/bin/env python3
"""The cost and the accuracy of FP8 (E4M3) head-major K / V shadows, one JSON line on stdout
(tools/kv_fp8_cost.py [--out profiles/kv_fp8_cost.json] [--widths 64,256,512]), in the manner of tools/kv_q4_cost.py.

Full-size TinyLlama, f16 weights and activations, synthetic, ctx 2048.  Per width, with the switch off and on IN THIS BUILD: the
attention launch at n = 2048 (in-library HIP-event timing of the family, us per launch; the K / V bytes it requests are (n - 1) x 128
or x 64 per kv head and sequence), the whole step (ms, wall clock over graph replays at n = 2040 .. 2047) and the import launch (ms
for one import of every sequence at n = 2048: the first step after a restart against the steps that follow).  Accuracy at 64
sequences: both decoders step through the same 256 ids from position 1; rms of the logit difference over the logit spread and the
share of equal greedy ids.  Nothing here is a threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTX, ATTN_FAMILY, F16 = 2048, 8, 1                             # KT_DEC_ATTN_SCORE (csrc/gten_rt.h), GTEN_F16


def batch_of(hip, host, S, fp8, ctx=CTX):
    cfg = host.default_config(F16, F16)
    cfg.max_ctx = ctx
    hip.set_kv_shadow_fp8(fp8)
    try:
        b = host.batch(cfg, S)
        b.load_synthetic(4242)
        b.decode_begin(0, host.synthetic_tokens(4, seed=1, n_vocab=cfg.n_vocab))
    finally:
        hip.set_kv_shadow_fp8(False)
    return cfg, b


def speed(hip, host, S):
    out = {}
    for name, fp8 in (("f16", False), ("fp8", True)):
        cfg, b = batch_of(hip, host, S, fp8)
        bits, chunk, total = b.kv_shadow_info()
        for q in range(S):
            b.decode_begin(q, host.synthetic_tokens(CTX, seed=10 + q, n_vocab=cfg.n_vocab))
        t0 = time.perf_counter()
        b.decode_step(2039, True)                              # (restarted: one import of every sequence, 2038 rows each)
        b.decode_result(0, 2039)
        t_first = time.perf_counter() - t0
        steps = []
        for rep in range(3):
            t0 = time.perf_counter()
            for n in range(2040, 2048):
                b.decode_step(n, True)
            b.decode_result(0, 2047)
            steps.append(1e3 * (time.perf_counter() - t0) / 8)
        us, launches = b.time_family(ATTN_FAMILY, CTX, 20)
        # (a step holds launches / n_layers attention launches per layer: lanes of 128 sequences above 128)
        kv_bytes = 2 * S * cfg.n_kv_heads * (CTX - 1) * (chunk // 256) * cfg.n_layers // launches
        out[name] = {"shadow_bits": bits, "chunk_bytes": chunk, "shadow_bytes": total, "attn_us": round(us, 2), "attn_launches": launches,
                     "attn_kv_bytes": kv_bytes, "attn_tb_per_s": round(kv_bytes / us * 1e-6, 3), "step_ms": round(min(steps), 4),
                     "step_ms_spread": round(max(steps) - min(steps), 4), "import_ms": round(1e3 * t_first - min(steps), 3)}
        b.close()
    out["attn_ratio_fp8_over_f16"] = round(out["fp8"]["attn_us"] / out["f16"]["attn_us"], 4)
    out["step_ratio_fp8_over_f16"] = round(out["fp8"]["step_ms"] / out["f16"]["step_ms"], 4)
    return out


def accuracy(hip, host, S=64, steps=256):
    logits = []
    for fp8 in (False, True):
        cfg, b = batch_of(hip, host, S, fp8, ctx=512)
        for q in range(S):
            b.decode_begin(q, host.synthetic_tokens(steps, seed=10 + q, n_vocab=cfg.n_vocab))
        rows = []
        for n in range(1, steps + 1):
            b.decode_step(n, True)
            rows.append(np.stack([b.logits(q) for q in (0, S // 2, S - 1)]))
        logits.append(np.stack(rows))
        b.close()
    a, c = logits[0].astype(np.float64), logits[1].astype(np.float64)
    rms = np.sqrt(((a - c) ** 2).mean(axis=-1)) / a.std(axis=-1)
    return {"sequences": S, "steps": steps, "rms_over_spread_mean": round(float(rms.mean()), 4), "rms_over_spread_max": round(float(rms.max()), 4),
            "greedy_agree": round(float((a.argmax(axis=-1) == c.argmax(axis=-1)).mean()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--widths", default="64,256,512")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    pkg = load_package()
    hip, host = pkg.hipabi.load(0), pkg.load_host()
    res = {"ctx": CTX, "weights": "f16", "widths": {}}
    for S in (int(x) for x in args.widths.split(",")):
        res["widths"][str(S)] = speed(hip, host, S)
        print(f"# {S}: {res['widths'][str(S)]}", file=sys.stderr, flush=True)
    res["accuracy"] = accuracy(hip, host)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
