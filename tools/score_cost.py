#!/usr/bin/env python3
"""The cost of scoring given ids, one JSON line on stdout (tools/score_cost.py [--out profiles/score_cost.json]).

Full-size TinyLlama, synthetic weights, q4, q8 and f16.  Per dtype: logits(tokens, 0) against score(tokens, 0) for a 2048-id
text (host clock around calls that end in a copy back, i.e. a synchronise; warmed up; median of --reps), the scored tok/s,
and score_many over two 2048-id windows.  Then the row kernel alone (gten_hip_row_logprobs) over 2048 x 32003 f32 rows at
the padded stride, timed by the in-library profiler (HIP events around each launch), with its effective bytes/s."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

N = 2048


def median_s(fn, reps):
    fn()                                                      # warm: graphs, kernels, scratch
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    pkg = load_package()
    hip = pkg.hipabi.load().init(0)
    host = pkg.load_host()
    res = {"n": N, "dtypes": {}}
    for name, wd, ad in (("q4", 4, 3), ("q8", 3, 3), ("f16", 1, 1)):
        m = host.model(host.default_config(wd, ad))
        m.load_synthetic(4242)
        toks = host.synthetic_tokens(N, seed=9, n_vocab=32003)
        t_logits = median_s(lambda: m.logits(toks, 0), a.reps)
        t_score = median_s(lambda: m.score(toks, 0), a.reps)
        w2 = [toks, host.synthetic_tokens(N, seed=10, n_vocab=32003)]
        t_many = median_s(lambda: m.score_many(w2), a.reps)
        res["dtypes"][name] = {"logits_ms": round(1e3 * t_logits, 3), "score_ms": round(1e3 * t_score, 3),
                               "score_over_logits": round(t_score / t_logits, 4), "scored_tok_per_s": round((N - 1) / t_score, 1),
                               "score_many_2x2048_ms": round(1e3 * t_many, 3),
                               "score_many_tok_per_s": round(2 * (N - 1) / t_many, 1)}
        m.close()
    V, stride = 32003, 32004
    r = np.random.default_rng(1)
    rows = (r.standard_normal((N, stride)) * 3).astype(np.float32)
    dev = hip.upload(rows)
    tg = r.integers(0, V, N).astype(np.int32)
    hip.row_logprobs(dev, N, V, stride, tg)                   # warm
    fam = hip.prof_family_index("row_logprobs")
    hip.prof_enable(True)
    for _ in range(a.reps):
        hip.row_logprobs(dev, N, V, stride, tg)
    hip.prof_enable(False)
    launches, total = hip.prof_read()["row_logprobs"]
    us = 1e3 * total / launches
    nbytes = N * V * 4
    res["row_kernel"] = {"family": fam, "rows": N, "n_vocab": V, "us": round(us, 2), "bytes": nbytes,
                         "tb_per_s": round(nbytes / (us * 1e-6) / 1e12, 3)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
