#!/usr/bin/env python3
"""The cost of a context shift, one JSON line on stdout
(tools/shift_cost.py [--out profiles/shift_cost.json] [--seqs 1,16,256] [--new 4096]).

Full-size TinyLlama geometry (22 layers, kv_dim 256, d_head 64), synthetic weights.
  launch      gten_hip_kv_shift alone on S sequences x 22 layers of plain device buffers, n = 2048, (keep, drop) = (64, 992), q8 and f16
              rows: ms per call (wall time of the call and a wait, best of 3 after a warm-up call) and the bytes read plus written per
              second -- every moved row of K and V once in, once out.  REPEATED LAUNCHES ON ONE BUFFER MAY HIT THE LAST-LEVEL CACHE:
              the small shapes fit it whole, so their rates say little about HBM;
  first_step  a 16-sequence q4 decoder at position 1024: an ordinary step, the first step after a shift of all 16 sequences (it pays
              the re-import of their head-major shadows) and the step after that, ms each;
  past_window generation of `new` ids behind a prompt of 256 on a single q4 model with a window of 2048: generate_shifting with
              (64, 992) against the only alternative without it -- whenever the window is full, the shortened ids go through the
              prompt path again (generate on ids[:64] + ids[1056:]) -- seconds each, and the shifts / re-prefills that took.
Nothing here is a threshold."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYERS, KV_DIM, D_HEAD, N, KEEP, DROP = 22, 256, 64, 2048, 64, 992


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def launch_cost(pkg, hip, S, dtype):
    rb = hip.row_bytes(dtype, KV_DIM)
    cache = N * rb
    buf = hip.alloc(S * LAYERS * 2 * cache)
    buf.zero()
    items = [(buf.ptr + (2 * i) * cache, buf.ptr + (2 * i + 1) * cache, N, KEEP, DROP) for i in range(S * LAYERS)]

    def call():
        hip.kv_shift(items, dtype, rb, KV_DIM, D_HEAD)
        hip.sync()
    call()
    s = min(timed(call) for _ in range(3))
    buf.free()
    moved = S * LAYERS * 2 * (N - KEEP - DROP) * rb * 2
    return {"sequences": S, "items": S * LAYERS, "ms": round(1e3 * s, 4), "bytes": moved, "gb_s": round(moved / s / 1e9, 1)}


def first_step_cost(pkg, host):
    cfg = host.default_config(4, 3)
    b = host.batch(cfg, 16)
    b.load_synthetic(1234)
    n = 1024
    ids = [host.synthetic_tokens(n + 8, seed=q, n_vocab=cfg.n_vocab) for q in range(16)]
    for q in range(16):
        b.decode_begin(q, ids[q])

    def step(at):
        return timed(lambda: (b.decode_step_ragged([at] * 16), b.decode_result(0, at)))
    step(n)
    ordinary = min(step(n + 1 + i) for i in range(3))
    t_shift = timed(lambda: (b.shift(list(range(16)), [n + 3] * 16, KEEP, 480), host.hip.sync()))
    for q in range(16):
        b.decode_begin(q, list(ids[q][:KEEP]) + list(ids[q][KEEP + 480:]))
    at = n + 4 - 480
    first = step(at)
    second = step(at + 1)
    out = {"sequences": 16, "ordinary_step_ms": round(1e3 * ordinary, 4), "shift_call_ms": round(1e3 * t_shift, 4),
           "first_step_after_ms": round(1e3 * first, 4), "second_step_after_ms": round(1e3 * second, 4), "head_major": bool(b.kv_info()[0])}
    b.close()
    return out


def past_window_cost(pkg, host, new):
    cfg = host.default_config(4, 3)
    m = host.model(cfg)
    m.load_synthetic(1234)
    prompt = [int(t) for t in host.synthetic_tokens(256, seed=3, n_vocab=cfg.n_vocab)]
    total = len(prompt) + new
    m.generate_shifting(prompt, 300, KEEP, DROP)                 # (warm-up: graphs captured)
    s0 = m.shift_info()[0]
    t_shift = timed(lambda: m.generate_shifting(prompt, total, KEEP, DROP))
    shifts = m.shift_info()[0] - s0

    def recompute():
        out, view, passes = list(prompt), list(prompt), 0
        while len(out) < total:
            got = [int(t) for t in m.generate(view, min(cfg.max_ctx + 1, len(view) + total - len(out)))]
            passes += 1
            out += got[len(view):]
            if len(got) == len(view):
                break
            view = got[:KEEP] + got[KEEP + DROP:]
        return passes
    passes = [0]
    t_re = timed(lambda: passes.__setitem__(0, recompute()))
    m.close()
    return {"new_ids": new, "window": cfg.max_ctx, "keep": KEEP, "drop": DROP, "shifting_s": round(t_shift, 4), "shifts": int(shifts),
            "recomputing_s": round(t_re, 4), "prompt_passes": passes[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seqs", default="1,16,256")
    ap.add_argument("--new", type=int, default=4096)
    a = ap.parse_args()
    from __graft_entry__ import load_package
    pkg = load_package()
    hip = pkg.hipabi.load(0)
    host = pkg.load_host()
    res = {"what": "context shift cost, TinyLlama-1.1B geometry, n 2048, (keep, drop) = (64, 992)",
           "note": "repeated launches on one buffer may hit the last-level cache", "launch": {"q8": [], "f16": []}}
    for S in [int(x) for x in a.seqs.split(",")]:
        res["launch"]["q8"].append(launch_cost(pkg, hip, S, pkg.hipabi.Q8))
        res["launch"]["f16"].append(launch_cost(pkg, hip, S, pkg.hipabi.F16))
    res["first_step"] = first_step_cost(pkg, host)
    res["past_window"] = past_window_cost(pkg, host, a.new)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
