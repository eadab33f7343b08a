#!/usr/bin/env python3
"""The cost of beam search on the device, one JSON line on stdout
(tools/beam_cost.py [--out profiles/beam_cost.json] [--shapes 1x4,2x4,16x4,32x8]).

Full-size TinyLlama, q4 weights, synthetic; prompts of 256 ids, max_new 64.  Per shape G x B (on a decoder of G * B sequences):
  ms_per_round    a whole search of 64 rounds minus one of 1 round, divided by 63: the prompt pass and the fan-out cancel.  It holds
                  the shared step, the lists (the step's own records, n_top = 2B), the round launch, the gather launch, the 4-byte
                  read of the live count and, on decoders with head-major shadows, the re-imports;
  step_ms         greedy generation's ms per step at the same width and context (no lists);
  step_lists_ms   the same with a log-prob request of n_top = 2B on every sequence: the lists' share is the difference;
  round_us        gten_hip_beam_round alone on G groups of random lists (the operator, 200 launches, one wait);
  permute         gten_hip_permute_sets alone on G * 22 * 2 ranges of B sets with 272-byte rows and a rotation as parent, at a tail of
                  1, 16 and 63 rows: bytes read plus written; launch_us and gb_s are the LAUNCH, timed by the library's event pairs
                  around it (20 launches); call_us is the wall time of the operator call, which also announces every base to the
                  watch registry and uploads its range table (72 bytes per range) -- host work the decoder form does once per search;
  imports_per_round   sequences re-imported into their shadows per round (0 on decoders that keep none).
Nothing here is a threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROMPT, MAX_NEW, ROW_BYTES, LAYERS = 256, 64, 272, 22


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def best(fn, repeats=3):
    return min(timed(fn) for _ in range(repeats))


def operators(pkg, hip, G, B):
    """(round_us, [permute at each tail])"""
    dev = lambda a: pkg.hipabi.DeviceBuffer.from_numpy(hip, np.ascontiguousarray(a))      # noqa: E731
    r = np.random.default_rng(G * 10 + B)
    garr = np.array([(g * B, B, 0, 1 << 20, -1) for g in range(G)], dtype=hip.BEAM_GROUP)
    ti = r.integers(0, 32000, (G * B, 16)).astype(np.int32)
    tl = -np.sort(r.random((G * B, 16)).astype(np.float32) * 6.0, axis=1)
    reps, rows = 200, 202
    d = [dev(garr), dev(np.zeros(G, hip.BEAM_STATE)), dev(ti), dev(tl), dev(np.ones(rows, np.float32)), dev(np.zeros((G, rows, 8), np.int32)),
         dev(np.zeros((G, rows, 8), np.int32)), dev(np.zeros(G * B, np.int32))]

    def rounds():
        hip._check(hip._memset(d[1].ptr, 0, d[1].nbytes))
        for _ in range(reps):
            hip.beam_round(d[0], d[1], d[2], d[3], 16, d[4], rows, d[5], d[6], rows, d[7])
        hip.sync()
    rounds()
    round_us = 1e6 * best(rounds) / reps
    out = []
    par = dev(np.tile(np.array([(b + 1) % B for b in range(B)] + [0] * (8 - B), np.int32), (G, 1)))
    for tail in (1, 16, 63):
        nbytes = tail * ROW_BYTES
        n_ranges = G * LAYERS * 2
        buf = pkg.hipabi.DeviceBuffer(hip, n_ranges * B * 63 * ROW_BYTES)
        ranges = [(i // (LAYERS * 2), [buf.ptr + (i * B + b) * 63 * ROW_BYTES for b in range(B)]) for i in range(n_ranges)]

        def launches():
            for _ in range(20):
                hip.permute_sets(ranges, 0, nbytes, d[0].ptr, G, None, par.ptr)
            hip.sync()
        launches()
        call_us = 1e6 * best(launches) / 20
        hip.prof_enable(True)                                     # (event pairs around every launch of the library from here on)
        launches()
        n, ms = hip.prof_read()["pack_weight"]                    # (the family the gather is filed under)
        hip.prof_enable(False)
        us = 1e3 * ms / n
        moved = 2 * n_ranges * B * nbytes
        out.append({"tail_rows": tail, "bytes": moved, "launch_us": round(us, 2), "gb_s": round(moved / us / 1e3, 1), "call_us": round(call_us, 2)})
    return round(round_us, 2), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="1x4,2x4,16x4,32x8")
    a = ap.parse_args()
    from __graft_entry__ import load_package
    pkg = load_package()
    hip = pkg.hipabi.load(0)
    host = pkg.load_host()
    cfg = host.default_config(4, 3)
    cfg.max_ctx = PROMPT + MAX_NEW + 2
    res = {"what": f"beam search cost, TinyLlama-1.1B q4 synthetic, prompts of {PROMPT} ids, max_new {MAX_NEW}", "shapes": {}}
    for shape in a.shapes.split(","):
        G, B = (int(x) for x in shape.split("x"))
        S = G * B
        b = host.batch(cfg, S)
        b.load_synthetic(4242)
        prompts = [list(host.synthetic_tokens(PROMPT, seed=10 + g, n_vocab=cfg.n_vocab)) for g in range(G)]
        every = [prompts[q // B] for q in range(S)]
        search = lambda n: b.beam_search(prompts, B, n)                                     # noqa: E731
        search(2)                                                                           # warm: graphs captured, prompt path compiled
        imports0 = b.kv_info()[1]
        search(MAX_NEW)
        imports_long = b.kv_info()[1] - imports0
        search(1)
        imports_short = b.kv_info()[1] - imports0 - imports_long
        ms_round = 1e3 * (best(lambda: search(MAX_NEW)) - best(lambda: search(1))) / (MAX_NEW - 1)
        total = PROMPT + MAX_NEW
        gen = lambda n: b.generate(every, n)                                                # noqa: E731
        gen(PROMPT + 2)
        step_ms = 1e3 * (best(lambda: gen(total)) - best(lambda: gen(PROMPT + 1))) / (MAX_NEW - 1)
        glp = lambda n: b.generate_logprobs(every, n, 2 * B)                                # noqa: E731
        glp(PROMPT + 2)
        step_lists_ms = 1e3 * (best(lambda: glp(total)) - best(lambda: glp(PROMPT + 1))) / (MAX_NEW - 1)
        head_major = bool(b.kv_info()[0])
        b.close()
        round_us, permute = operators(pkg, hip, G, B)
        res["shapes"][shape] = {"sequences": S, "ms_per_round": round(ms_round, 4), "step_ms": round(step_ms, 4), "step_lists_ms": round(step_lists_ms, 4),
                                "round_us": round_us, "permute": permute, "head_major": head_major,
                                "imports_per_round": round((imports_long - imports_short) / (MAX_NEW - 1), 2)}
        print(shape, json.dumps(res["shapes"][shape]), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
