#!/usr/bin/env python3
"""What a shared prompt prefix buys on the serving queue, one JSON line on stdout
(tools/prefix_cost.py [--out profiles/prefix_cost.json] [--merge FILE ...]).

Without --step this is a driver: it runs the steps below one after the other, each as a child process of its own under
`timeout` (one process on the GPU at a time), stops at the first one that fails, and merges their results.

  --step kernels   one full-size block (q4 weights, Q8 activations), the rows that follow a 256-id prefix in as many
                   prompts of 64..256 ids as fit 4096 rows: per-layer time of the batched RoPE and attention launches
                   (HIP events of the in-library profiler), the per-segment launches of the plain path on the same rows,
                   and the whole prompts (prefix + their rows) the plain way; wall time of the whole block call for each.
  --step serve     full-size synthetic q4, 256 slots, a queue of 1024 prompts -- the 256-id prefix plus 64..256 ids of
                   their own, budgets of 32..224 new ids: served with the prefix unset and set, three times each in
                   alternation: new tok/s, prefill_s, rows computed; the ids of both ways compared.
                   On a build without the feature (the parent commit) only the unset runs are made: the baseline.
  --step decode    the DECODE side (decode slots behind the prefix read one copy of its K / V, include/gten_hip_prefix_decode.h):
                   full-size synthetic q4, 256 slots, a 1024-id prefix plus 64..256 ids of their own, the prefix set both ways and
                   gten_hip_set_prefix_decode_shared off / on, three times each in alternation: (a) the attention family's launch
                   time (gten_hip_decoder_time_family at the longest context), (b) ms per shared ragged step.
  --step serve_decode   (c) the serving queue of --step serve behind the 1024-id prefix, the switch off / on, three runs each in
                   alternation: new tok/s, and the ids of both ways compared.
  (--decode: the driver runs these two instead of kernels and serve; results go to profiles/prefix_decode_cost.json)
  --step prefixes  SEVERAL prefixes (include/gten_host_prefixes.h; --prefixes K, default 4): full-size synthetic q4, 256 slots, K
                   prefixes of 1024 ids with 256 / K slots behind each: the shared ragged step and the attention family's launch
                   with gten_hip_set_prefix_decode_shared off / on, three runs each in alternation -- and, on the same build and
                   in the same alternation, today's best case: ONE 1024-id prefix behind all 256 slots.
  --step serve_prefixes   the serving queue of 1024 prompts split over the K prefixes, all K registered against only index 0
                   registered (what a build with one prefix can do), three runs each in alternation; the ids compared.
  (--prefixes K: the driver runs these two; results go to profiles/prefixes_cost.json)
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

PREFIX, SLOTS, QUEUE, CTX, REPS = 256, 256, 1024, 2048, 3
STEP_LIMIT_S = {"kernels": 240, "serve": 600, "decode": 420, "serve_decode": 600, "prefixes": 540, "serve_prefixes": 600}
DEC_PREFIX = 1024
N_PREFIXES = 4


def queue(host, cfg, n_prefix=PREFIX):
    rng = np.random.default_rng(2025)
    own = rng.integers(64, 257, QUEUE)
    budgets = rng.integers(32, 225, QUEUE).astype(np.int32)
    prefix = [int(t) for t in host.synthetic_tokens(n_prefix, seed=424242, n_vocab=cfg.n_vocab)]
    prompts = [prefix + [int(t) for t in host.synthetic_tokens(int(n), seed=9000 + j, n_vocab=cfg.n_vocab)] for j, n in enumerate(own)]
    return prefix, prompts, budgets


def step_serve():
    pkg = load_package()
    pkg.hipabi.load(0)
    host = pkg.load_host()
    cfg = host.default_config(4, 3)
    cfg.max_ctx = CTX
    b = host.batch(cfg, SLOTS)
    b.load_synthetic(4242)
    prefix, prompts, budgets = queue(host, cfg)
    has = hasattr(b, "set_prefix")
    res = {"slots": SLOTS, "prompts": QUEUE, "prefix_ids": PREFIX, "own_ids": "64..256", "feature_in_build": has, "runs": []}
    b.serve(prompts[:SLOTS], CTX, -1, 8, max_new=4)                       # warm-up: graphs, first-use allocations
    if has:
        b.set_prefix(prefix)
        b.serve(prompts[:SLOTS], CTX, -1, 8, max_new=4)
        b.set_prefix(None)
    ids = {}
    for rep in range(REPS):
        for mode in (("unset", "set") if has else ("unset",)):
            rows0 = 0
            if has:
                b.set_prefix(prefix if mode == "set" else None)
                rows0 = b.prefix_info()[2]
            t0 = time.perf_counter()
            got, st = b.serve(prompts, CTX, -1, 8, max_new_each=budgets)
            wall = time.perf_counter() - t0
            run = {"prefix": mode, "rep": rep, "new_tok_s": round(st["new_tokens"] / wall, 1), "wall_s": round(wall, 4),
                   "prefill_s": round(st["prefill_s"], 4), "decode_s": round(st["decode_s"], 4), "new_tokens": int(st["new_tokens"]),
                   "prompt_tokens": int(st["prompt_tokens"])}
            if has:
                run["rows_computed"] = int(b.prefix_info()[2] - rows0)
            res["runs"].append(run)
            ids.setdefault(mode, got)
    if has:
        b.set_prefix(None)
        res["same_ids_set_and_unset"] = bool(all(np.array_equal(x, y) for x, y in zip(ids["unset"], ids["set"])))
    for mode in ids:
        r = [x for x in res["runs"] if x["prefix"] == mode]
        res[mode] = {"new_tok_s_median": float(np.median([x["new_tok_s"] for x in r])), "new_tok_s_min_max": [min(x["new_tok_s"] for x in r), max(x["new_tok_s"] for x in r)],
                     "prefill_s_median": float(np.median([x["prefill_s"] for x in r])), "rows_computed": r[0].get("rows_computed")}
    b.close()
    return res


def spread(values):
    return {"median": round(float(np.median(values)), 4), "min_max": [round(float(min(values)), 4), round(float(max(values)), 4)]}


def full_size_batch():
    pkg = load_package()
    hip = pkg.hipabi.load(0)
    host = pkg.load_host()
    cfg = host.default_config(4, 3)
    cfg.max_ctx = CTX
    b = host.batch(cfg, SLOTS)
    b.load_synthetic(4242)
    return hip, host, cfg, b


def step_decode():
    hip, host, cfg, b = full_size_batch()
    prefix, prompts, _ = queue(host, cfg, DEC_PREFIX)
    prompts = prompts[:SLOTS]
    steps = 32
    streams = [p + [int(t) for t in host.synthetic_tokens(steps + 8, seed=7000 + q, n_vocab=cfg.n_vocab)] for q, p in enumerate(prompts)]
    fam = hip.prof_family_index("decode_attn_score")
    n_long = max(len(p) for p in prompts) + 1
    b.set_prefix(prefix)
    res = {"slots": SLOTS, "prefix_ids": DEC_PREFIX, "own_ids": "64..256", "steps_timed": steps, "attention_family_context": n_long, "runs": []}
    last = {}
    for rep in range(REPS + 1):                                            # (rep 0: warm-up -- graphs, first-use allocations)
        for mode in ("off", "on"):
            host.set_prefix_decode_shared(mode == "on")
            for i in range(0, SLOTS, 3):                                   # (a call takes 4096 ids: three prompts of at most 1280)
                b.prefill_many(list(range(i, min(i + 3, SLOTS))), prompts[i:i + 3], want=False)
            for q, s_ in enumerate(streams):
                b.decode_begin(q, s_)
            sharing = sum(1 for q in range(SLOTS) if b.prefix_decode_info(q)[1] > 0)
            for t in (1, 2):                                               # (imports, graph capture)
                b.decode_step_ragged([len(p) + t for p in prompts], use_graph=True)
            hip.sync()
            t0 = time.perf_counter()
            for t in range(3, 3 + steps):
                b.decode_step_ragged([len(p) + t for p in prompts], use_graph=True)
            hip.sync()
            ms = 1e3 * (time.perf_counter() - t0) / steps
            last[mode] = np.stack([b.logits(q) for q in (0, 1, SLOTS // 2, SLOTS - 1)])
            us, launches = b.time_family(fam, n_long, 20)
            if rep:
                res["runs"].append({"shared": mode, "rep": rep, "ms_per_step": round(ms, 4), "attn_launch_us": round(us, 2),
                                    "attn_launches_per_step": launches, "sequences_sharing": sharing})
    host.set_prefix_decode_shared(None)
    res["same_logits_on_and_off"] = bool(np.array_equal(last["off"], last["on"]))
    for mode in ("off", "on"):
        r = [x for x in res["runs"] if x["shared"] == mode]
        res[mode] = {"ms_per_step": spread([x["ms_per_step"] for x in r]), "attn_launch_us": spread([x["attn_launch_us"] for x in r]),
                     "sequences_sharing": r[0]["sequences_sharing"]}
    b.close()
    return res


def step_serve_decode():
    hip, host, cfg, b = full_size_batch()
    prefix, prompts, budgets = queue(host, cfg, DEC_PREFIX)
    b.set_prefix(prefix)
    res = {"slots": SLOTS, "prompts": QUEUE, "prefix_ids": DEC_PREFIX, "own_ids": "64..256", "runs": []}
    for mode in ("off", "on"):                                             # warm-up
        host.set_prefix_decode_shared(mode == "on")
        b.serve(prompts[:SLOTS], CTX, -1, 8, max_new=4)
    ids = {}
    for rep in range(REPS):
        for mode in ("off", "on"):
            host.set_prefix_decode_shared(mode == "on")
            skip0 = b.prefix_decode_info()[3]
            t0 = time.perf_counter()
            got, st = b.serve(prompts, CTX, -1, 8, max_new_each=budgets)
            wall = time.perf_counter() - t0
            res["runs"].append({"shared": mode, "rep": rep, "new_tok_s": round(st["new_tokens"] / wall, 1), "wall_s": round(wall, 4),
                                "prefill_s": round(st["prefill_s"], 4), "decode_s": round(st["decode_s"], 4), "new_tokens": int(st["new_tokens"]),
                                "imports_skipping_shared_chunks": int(b.prefix_decode_info()[3] - skip0)})
            ids.setdefault(mode, got)
    host.set_prefix_decode_shared(None)
    res["same_ids_on_and_off"] = bool(all(np.array_equal(x, y) for x, y in zip(ids["off"], ids["on"])))
    for mode in ("off", "on"):
        r = [x["new_tok_s"] for x in res["runs"] if x["shared"] == mode]
        res[mode] = {"new_tok_s": spread(r)}
    b.close()
    return res


def queue_over(host, cfg, k):
    """queue()'s own ids and budgets behind K different 1024-id prefixes, prompt j behind prefix j % K"""
    rng = np.random.default_rng(2025)
    own = rng.integers(64, 257, QUEUE)
    budgets = rng.integers(32, 225, QUEUE).astype(np.int32)
    prefixes = [[int(t) for t in host.synthetic_tokens(DEC_PREFIX, seed=424242 + 1000 * w, n_vocab=cfg.n_vocab)] for w in range(k)]
    prompts = [prefixes[j % k] + [int(t) for t in host.synthetic_tokens(int(n), seed=9000 + j, n_vocab=cfg.n_vocab)] for j, n in enumerate(own)]
    return prefixes, prompts, budgets


def step_prefixes():
    hip, host, cfg, b = full_size_batch()
    k = N_PREFIXES
    prefixes, prompts_k, _ = queue_over(host, cfg, k)
    _, prompts_1, _ = queue_over(host, cfg, 1)                            # (the same own ids, all behind prefix 0)
    steps = 32
    fam = hip.prof_family_index("decode_attn_score")
    res = {"slots": SLOTS, "prefixes": k, "prefix_ids": DEC_PREFIX, "own_ids": "64..256", "steps_timed": steps, "runs": []}
    cases = (("off", k, False), ("one_prefix", 1, True), ("on", k, True))
    last = {}
    for rep in range(REPS + 1):                                            # (rep 0: warm-up -- graphs, first-use allocations)
        for name, n_reg, shared in cases:
            prompts = (prompts_k if n_reg == k else prompts_1)[:SLOTS]
            n_long = max(len(p) for p in prompts) + 1
            for w in range(k):
                b.set_prefix_at(w, prefixes[w] if w < n_reg else None)
            host.set_prefix_decode_shared(shared)
            for i in range(0, SLOTS, 3):                                   # (a call takes 4096 ids: three prompts of at most 1280)
                b.prefill_many(list(range(i, min(i + 3, SLOTS))), prompts[i:i + 3], want=False)
            streams = [p + [int(t) for t in host.synthetic_tokens(steps + 8, seed=7000 + q, n_vocab=cfg.n_vocab)] for q, p in enumerate(prompts)]
            for q, s_ in enumerate(streams):
                b.decode_begin(q, s_)
            sharing = [sum(1 for q in range(SLOTS) if b.prefix_decode_info_at(q) == (w, DEC_PREFIX // 256)) for w in range(k)]
            for t in (1, 2):                                               # (imports, graph capture)
                b.decode_step_ragged([len(p) + t for p in prompts], use_graph=True)
            hip.sync()
            t0 = time.perf_counter()
            for t in range(3, 3 + steps):
                b.decode_step_ragged([len(p) + t for p in prompts], use_graph=True)
            hip.sync()
            ms = 1e3 * (time.perf_counter() - t0) / steps
            if n_reg == k:
                last[name] = np.stack([b.logits(q) for q in (0, 1, SLOTS // 2, SLOTS - 1)])
            us, launches = b.time_family(fam, n_long, 20)
            if rep:
                res["runs"].append({"case": name, "rep": rep, "ms_per_step": round(ms, 4), "attn_launch_us": round(us, 2),
                                    "attn_launches_per_step": launches, "sequences_sharing_per_prefix": sharing})
    host.set_prefix_decode_shared(None)
    res["same_logits_on_and_off"] = bool(np.array_equal(last["off"], last["on"]))
    for name, _, _ in cases:
        r = [x for x in res["runs"] if x["case"] == name]
        res[name] = {"ms_per_step": spread([x["ms_per_step"] for x in r]), "attn_launch_us": spread([x["attn_launch_us"] for x in r]),
                     "sequences_sharing_per_prefix": r[0]["sequences_sharing_per_prefix"]}
    b.close()
    return res


def step_serve_prefixes():
    hip, host, cfg, b = full_size_batch()
    k = N_PREFIXES
    prefixes, prompts, budgets = queue_over(host, cfg, k)
    res = {"slots": SLOTS, "prompts": QUEUE, "prefixes": k, "prefix_ids": DEC_PREFIX, "own_ids": "64..256", "runs": []}

    def register(n_reg):
        for w in range(k):
            b.set_prefix_at(w, prefixes[w] if w < n_reg else None)

    for n_reg in (1, k):                                                   # warm-up
        register(n_reg)
        b.serve(prompts[:SLOTS], CTX, -1, 8, max_new=4)
    ids = {}
    for rep in range(REPS):
        for name, n_reg in (("index_0_only", 1), ("all", k)):
            register(n_reg)
            sh0 = [b.prefixes_info(w)[1] for w in range(k)]
            rows0 = b.prefix_info()[2]
            t0 = time.perf_counter()
            got, st = b.serve(prompts, CTX, -1, 8, max_new_each=budgets)
            wall = time.perf_counter() - t0
            res["runs"].append({"registered": name, "rep": rep, "new_tok_s": round(st["new_tokens"] / wall, 1), "wall_s": round(wall, 4),
                                "prefill_s": round(st["prefill_s"], 4), "decode_s": round(st["decode_s"], 4), "new_tokens": int(st["new_tokens"]),
                                "rows_computed": int(b.prefix_info()[2] - rows0),
                                "prompts_shared_per_prefix": [int(b.prefixes_info(w)[1] - sh0[w]) for w in range(k)]})
            ids.setdefault(name, got)
    register(0)
    res["same_ids_both_ways"] = bool(all(np.array_equal(x, y) for x, y in zip(ids["index_0_only"], ids["all"])))
    for name in ids:
        r = [x for x in res["runs"] if x["registered"] == name]
        res[name] = {"new_tok_s": spread([x["new_tok_s"] for x in r]), "rows_computed": r[0]["rows_computed"]}
    b.close()
    return res


def step_kernels():
    pkg = load_package()
    hip = pkg.hipabi.load(0)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle import orc
    orc.build(ref=False)
    oracle = orc.load_oracle()
    from helpers import Q4, Q8, act_rows, rng, row_bytes
    from test_block_rows_gpu import alloc_acts, make_block
    E, H, KVH, F = 2048, 32, 4, 5632
    r = rng(11)
    w, widths = make_block(hip, oracle, r, Q4, E, H, KVH, F, 0)
    own = []
    for n in np.random.default_rng(2025).integers(64, 257, 64):
        if sum(own) + int(n) > 4096:
            break
        own.append(int(n))
    n_suf = sum(own)
    ints = dict(adtype=Q8, wdtype=Q4, n_embd=E, n_heads=H, n_kv_heads=KVH, n_ffn=F)
    rows = act_rows(oracle, r, PREFIX + n_suf, E, Q8)[0]
    pre_rows, suf_rows = rows[:PREFIX], rows[PREFIX:]
    starts = [0] + [int(x) for x in np.cumsum(own)]

    def bufs_for(n, inp):
        bufs = dict(w)
        bufs.update(alloc_acts(hip, widths, n, 0, Q8))
        bufs["inp"] = hip.upload(inp)
        return bufs

    b_pre = bufs_for(PREFIX, pre_rows)
    hip.set_row_segments([0, PREFIX])
    assert hip.block_rows(PREFIX, 0, ints, b_pre)
    b_suf = bufs_for(n_suf, suf_rows)
    # the whole prompts the plain way, in calls of at most 4096 rows
    groups, cur = [], []
    for k, n in enumerate(own):
        if sum(PREFIX + own[i] for i in cur) + PREFIX + n > 4096:
            groups.append(cur)
            cur = []
        cur.append(k)
    groups.append(cur)
    whole = []
    for g in groups:
        inp = np.concatenate([np.concatenate([pre_rows, suf_rows[starts[k]:starts[k + 1]]]) for k in g])
        st = [0] + [int(x) for x in np.cumsum([PREFIX + own[k] for k in g])]
        whole.append((st, bufs_for(st[-1], inp)))

    def prefixed():
        hip.set_row_segments(starts)
        assert hip.block_rows_prefixed(n_suf, ints, b_suf, b_pre["k"], b_pre["v"], PREFIX)

    def plain_suffixes():
        hip.set_row_segments(starts)
        assert hip.block_rows(n_suf, 0, ints, b_suf)

    def plain_whole():
        for st, bufs in whole:
            hip.set_row_segments(st)
            assert hip.block_rows(st[-1], 0, ints, bufs)

    def measure(fn, reps=20):
        fn()
        hip.sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        hip.sync()
        wall_us = 1e6 * (time.perf_counter() - t0) / reps
        hip.prof_enable(True)
        fn()
        prof = hip.prof_read()
        hip.prof_enable(False)
        out = {"block_wall_us": round(wall_us, 1)}
        for fam, key in (("rotary_emb", "rope"), ("qkv_attn_tiled", "attention")):
            n, ms = prof.get(fam, (0, 0.0))
            out[key] = {"launches": n, "us": round(1e3 * ms, 1)}
        out["all_launches_us"] = round(1e3 * sum(ms for _, ms in prof.values()), 1)
        return out

    res = {"prompts": len(own), "rows_after_the_prefix": n_suf, "prefix_ids": PREFIX, "whole_prompt_calls": len(groups),
           "prefixed": measure(prefixed), "plain_on_the_same_rows_no_prefix": measure(plain_suffixes), "whole_prompts_plain": measure(plain_whole)}
    hip.set_row_segments(None)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S), default=None)
    ap.add_argument("--decode", action="store_true", help="the decode side: steps decode and serve_decode")
    ap.add_argument("--prefixes", type=int, default=0, metavar="K", help="several prefixes (2..8): steps prefixes and serve_prefixes")
    ap.add_argument("--merge", nargs="*", default=[], help="name=file.json: results measured elsewhere (the parent commit's runs) recorded beside these")
    a = ap.parse_args()
    global N_PREFIXES
    if a.prefixes:
        if not 2 <= a.prefixes <= 8 or SLOTS % a.prefixes:
            ap.error("--prefixes: 2, 4 or 8")
        N_PREFIXES = a.prefixes
    if a.step:
        res = {"serve": step_serve, "kernels": step_kernels, "decode": step_decode, "serve_decode": step_serve_decode,
               "prefixes": step_prefixes, "serve_prefixes": step_serve_prefixes}[a.step]()
        print(json.dumps(res))
        return 0
    res = {"what": "shared prompt prefix, TinyLlama-1.1B q4 synthetic, %d slots, %d prompts = %d shared ids + 64..256 of their own" % (SLOTS, QUEUE, PREFIX)}
    if a.decode:
        res["what"] = "decode slots behind a shared prefix read one copy of its K / V, TinyLlama-1.1B q4 synthetic, %d slots, %d shared ids + 64..256 of their own" % (SLOTS, DEC_PREFIX)
    if a.prefixes:
        res["what"] = "%d shared prefixes at once, TinyLlama-1.1B q4 synthetic, %d slots, %d shared ids + 64..256 of their own, %d slots behind each" % (
            N_PREFIXES, SLOTS, DEC_PREFIX, SLOTS // N_PREFIXES)
    for step in (("prefixes", "serve_prefixes") if a.prefixes else ("decode", "serve_decode") if a.decode else ("kernels", "serve")):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + (["--prefixes", str(N_PREFIXES)] if a.prefixes else [])
        p = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S[step])] + cmd,
                           capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            sys.stderr.write("\nprefix_cost: step %s ended with %d: stopping\n" % (step, p.returncode))
            return 1
        res[step] = json.loads(p.stdout.strip().splitlines()[-1])
    for item in a.merge:
        name, path = item.split("=", 1)
        with open(path) as f:
            res[name] = json.load(f)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
