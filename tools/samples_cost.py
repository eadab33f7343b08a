#!/usr/bin/env python3
"""What n samples per prompt cost on the serving queue, one JSON line on stdout
(tools/samples_cost.py [--out profiles/samples_cost.json] [--prompts 256] [--samples 4] [--reps 3]).

Full-size synthetic q4, 256 slots, a queue of 256 prompts of 256..768 ids, four samples each, budgets of 32..224 new ids, sampled
(top-k 40, T 0.9).  Three ways in alternation, --reps runs each, reported as median and min-max:

  expanded   the expanded queue -- every prompt written out four times -- through the existing call (serve_fsm);
  passes     serve_samples with set_groups_cap(0): the prompt passes are saved, every member decodes on its own copy;
  records    serve_samples with set_groups_cap(64): the members also read the prompt's full chunks from one group record.

Per way: new tok/s, prefill_s, prompt rows computed and ms per shared step; the ids of the three ways are compared.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

SLOTS, CTX = 256, 1024


def spread(values):
    return {"median": round(float(np.median(values)), 4), "min_max": [round(float(min(values)), 4), round(float(max(values)), 4)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--prompts", type=int, default=256)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    pkg = load_package()
    pkg.hipabi.load(0)
    host = pkg.load_host()
    cfg = host.default_config(4, 3)
    cfg.max_ctx = CTX
    b = host.batch(cfg, SLOTS)
    b.load_synthetic(4242)
    rng = np.random.default_rng(2026)
    lens = rng.integers(256, 769, args.prompts)
    prompts = [[int(t) for t in host.synthetic_tokens(int(n), seed=7000 + j, n_vocab=cfg.n_vocab)] for j, n in enumerate(lens)]
    ns = [args.samples] * args.prompts
    budgets = rng.integers(32, 225, args.prompts * args.samples).astype(np.int32)      # per item of the expanded queue
    items = [p for p in prompts for _ in range(args.samples)]
    seed = 99

    def expanded():
        ids, st, _ = b.serve_fsm(items, CTX, -1, 40, 0.9, seed, -1, slice_steps=8, max_new_each=budgets)
        return ids, st

    def samples(cap):
        b.set_groups_cap(cap)
        try:
            ids, st, _ = b.serve_samples_items(prompts, ns, CTX, -1, 40, 0.9, seed, slice_steps=8, max_new_each=budgets)      # (a budget per item)
        finally:
            b.set_groups_cap(-1)
        return ids, st

    ways = {"expanded": expanded, "passes": lambda: samples(0), "records": lambda: samples(host.GROUPS_MAX)}
    warm = [p[:300] for p in prompts[: SLOTS // args.samples]]
    b.serve_fsm([p for p in warm for _ in range(args.samples)], CTX, -1, 40, 0.9, seed, -1, slice_steps=8, max_new=4)     # graphs, first-use allocations
    b.set_groups_cap(host.GROUPS_MAX)
    b.serve_samples_items(warm, [args.samples] * len(warm), CTX, -1, 40, 0.9, seed, slice_steps=8, max_new=4)
    b.set_groups_cap(-1)
    res = {"slots": SLOTS, "prompts": args.prompts, "samples": args.samples, "prompt_ids": "256..768", "budgets": "32..224", "ctx": CTX, "runs": []}
    ids = {}
    for rep in range(args.reps):
        for way, fn in ways.items():
            rows0, info0 = b.prefix_info()[2], b.samples_info()
            t0 = time.perf_counter()
            got, st = fn()
            wall = time.perf_counter() - t0
            info = [a - c for a, c in zip(b.samples_info(), info0)]
            res["runs"].append({"way": way, "rep": rep, "new_tok_s": round(st["new_tokens"] / wall, 1), "wall_s": round(wall, 4),
                                "prefill_s": round(st["prefill_s"], 4), "decode_s": round(st["decode_s"], 4), "steps": int(st["steps"]),
                                "ms_per_step": round(1e3 * st["decode_s"] / max(st["steps"], 1), 4), "new_tokens": int(st["new_tokens"]),
                                "rows_computed": int(b.prefix_info()[2] - rows0), "copies": int(info[0]), "groups_recorded": int(info[2]),
                                "groups_unrecorded": int(info[3])})
            ids.setdefault(way, got)
    for way in ways:
        r = [x for x in res["runs"] if x["way"] == way]
        res[way] = {"new_tok_s": spread([x["new_tok_s"] for x in r]), "prefill_s": spread([x["prefill_s"] for x in r]),
                    "ms_per_step": spread([x["ms_per_step"] for x in r]), "rows_computed": r[0]["rows_computed"]}
    res["same_ids"] = bool(all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in zip(ids["expanded"], ids["passes"], ids["records"])))
    b.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
