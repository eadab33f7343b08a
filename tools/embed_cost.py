#!/usr/bin/env python3
"""The cost of embeddings, one JSON line on stdout
(tools/embed_cost.py [--out profiles/embed_cost.json] [--texts 256] [--calls 200] [--repeats 7] [--bench-ab FILE]).

  pool        gten_hip_pool_rows on plain device buffers at 32 texts x 128 rows and 2 texts x 2048 rows (4096 rows each), q8 and f16 rows,
              n_embd 2048, mean and last pooling, normalised: us per call.  Beside it gten_hip_rms_norm over the same 4096 rows -- the
              final norm that reads the same matrix (and writes one of its size) -- timed in the same way.  A figure is the wall time of
              `calls` back-to-back calls and one wait, per call; `repeats` such windows after a warm-up, reported as min / median / max.
              REPEATED LAUNCHES ON ONE 9 MB MATRIX FIND IT IN THE LAST-LEVEL CACHE: these are launch and latency figures, not HBM rates;
  many        embed_many over `texts` synthetic texts of 64..256 ids on the full-size q4 model, beside score_many on the same texts (what
              a caller had before: the same prompt passes, then the lm_head of every row): seconds per call, texts / s and ids / s as
              min / median / max of `repeats` calls after a warm-up, and the launches of one call of each, counted by the library's
              profiler in a separate call.
  bench       with --bench-ab FILE: the values of `bench.py` runs of the parent's build and of this tree, alternating processes, read from
              FILE (one line per run: `parent` or `tree`, a blank, the run's JSON line) -- this tool cannot build the parent itself.
Nothing here is a threshold."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

E = 2048
SHAPES = ((32, 128), (2, 2048))


def spread(xs, digits=3):
    return {"min": round(min(xs), digits), "median": round(statistics.median(xs), digits), "max": round(max(xs), digits)}


def window(hip, fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    hip.sync()
    return (time.perf_counter() - t0) / calls


def pool_cost(pkg, hip, dtype, calls, repeats):
    rb = hip.row_bytes(dtype, E)
    rows = 4096
    r = np.random.default_rng(1)
    if dtype == pkg.hipabi.F16:
        mat = r.standard_normal((rows, E)).astype(np.float16).view(np.uint8).reshape(rows, rb)
    else:
        mat = np.zeros((rows, E // 32, 34), np.uint8)
        mat[:, :, :2] = r.uniform(0.01, 0.05, (rows, E // 32)).astype(np.float16).view(np.uint8).reshape(rows, E // 32, 2)
        mat[:, :, 2:] = r.integers(-127, 128, (rows, E // 32, 32)).astype(np.int8).view(np.uint8)
        mat = mat.reshape(rows, rb)
    x = hip.upload(mat)
    normed = hip.alloc(rows * rb)
    w = hip.upload(np.ones(E, np.float16))
    out = hip.alloc(4 * 32 * E)
    res = {"rows": rows, "row_bytes": rb, "matrix_bytes": rows * rb}

    def timed(fn):
        window(hip, fn, calls)
        return spread([1e6 * window(hip, fn, calls) for _ in range(repeats)], 2)
    res["rms_norm_us"] = timed(lambda: hip.rms_norm(x, dtype, w, normed, rows, E, 0))
    for T, n in SHAPES:
        starts = [k * n for k in range(T + 1)]
        for pooling in ("mean", "last"):
            res[f"pool_{pooling}_{T}x{n}_us"] = timed(lambda: hip._check(hip.pool_rows_rc(x, dtype, rb, E, starts, pooling, True, out)))
    for b in (x, normed, w, out):
        b.free()
    return res


def many_cost(pkg, hip, host, n_texts, repeats):
    cfg = host.default_config(pkg.hipabi.Q4, pkg.hipabi.Q8)
    m = host.model(cfg)
    m.load_synthetic(1234)
    r = np.random.default_rng(3)
    texts = [host.synthetic_tokens(int(n), seed=500 + i, n_vocab=cfg.n_vocab) for i, n in enumerate(r.integers(64, 257, n_texts))]
    ids = int(sum(len(t) for t in texts))

    def timed(fn):
        fn()
        xs = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            fn()
            xs.append(time.perf_counter() - t0)
        return xs

    def launches(fn):
        hip.prof_enable(True)
        hip.prof_read()
        before = {k: v[0] for k, v in hip.prof_read().items()}
        fn()
        hip.sync()
        after = {k: v[0] for k, v in hip.prof_read().items()}
        hip.prof_enable(False)
        by = {k: after[k] - before.get(k, 0) for k in after if after[k] - before.get(k, 0)}
        return sum(by.values()), by
    out = {"texts": n_texts, "ids": ids, "groups": len(host.embed_plan([len(t) for t in texts])[1])}
    for name, fn in (("embed_many", lambda: m.embed_many(texts)), ("score_many", lambda: m.score_many(texts))):
        xs = timed(fn)
        n, by = launches(fn)
        out[name] = {"s": spread(xs, 4), "texts_per_s": spread([n_texts / x for x in xs], 1), "ids_per_s": spread([ids / x for x in xs], 0),
                     "launches": n, "launches_by_family": by}
    m.close()
    return out


def bench_ab(path):
    vals = {"parent": [], "tree": []}
    for ln in open(path):
        which, line = ln.split(" ", 1)
        vals[which].append(json.loads(line)["value"])
    return {"command": "bench.py --gpus 1 --steps 256 --warmup 32, processes alternating parent / tree", "unit": "tok/s",
            **{k: {"runs": v, "min": min(v), "max": max(v), "mean": round(sum(v) / len(v), 2)} for k, v in vals.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--texts", type=int, default=256)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--bench-ab", default=None)
    a = ap.parse_args()
    from __graft_entry__ import load_package
    pkg = load_package()
    hip = pkg.hipabi.load(0)
    host = pkg.load_host()
    res = {"what": "embedding cost: gten_hip_pool_rows beside the final norm over the same 4096 x 2048 rows; embed_many beside score_many, full-size q4",
           "note": "pool / norm: wall time of back-to-back calls and one wait, per call; the 9 MB matrix stays in the last-level cache",
           "pool": {"q8": pool_cost(pkg, hip, pkg.hipabi.Q8, a.calls, a.repeats), "f16": pool_cost(pkg, hip, pkg.hipabi.F16, a.calls, a.repeats)},
           "many": many_cost(pkg, hip, host, a.texts, a.repeats)}
    if a.bench_ab:
        res["bench"] = bench_ab(a.bench_ab)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
