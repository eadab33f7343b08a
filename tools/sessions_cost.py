#!/usr/bin/env python3
"""What continuing a conversation costs against recomputing it, one JSON line on stdout
(tools/sessions_cost.py [--out profiles/sessions_cost.json]).

Without --step this is a driver: it runs the steps below one after the other, each as a child process of its own under
`timeout` (one process on the GPU at a time), stops at the first one that fails, and merges their results.

  --step attention  (the continued call's wall time includes its table upload, which a model pays once for all its layers)
                    one full-size block (q4 weights, Q8 activations): 32 segments of 32..96 new rows behind contexts of their
                    own of 300..1500 rows through gten_hip_block_rows_continued, and the same row counts behind ONE 1024-row
                    prefix through gten_hip_block_rows_prefixed: per-layer time of the RoPE and attention launches (HIP events
                    of the in-library profiler) and wall time of the whole block call.
  --step extend     full-size synthetic q4, 256 sequences of max_ctx 2048 that hold a first turn (a prompt of 256..512 ids and 64
                    more): a second turn of 32..96 ids (a) through extend_many -- only its rows are computed -- and (b) the same
                    build processing history + turn as fresh prompts through prefill_many, today's only way; three runs each
                    in alternation: wall seconds, rows computed, turn ids per second (no logits copied back either way); the turns'
                    first ids of both ways compared once, outside the timed runs.
  --step serve      THE QUEUE: full-size synthetic q4, 256 slots and 256 sessions; turn 1 = prompts of 256..512 ids and 64 new ids
                    through serve_sessions (not timed); turn 2 = 32..96 ids and 64 new ids (a) through serve_sessions on those
                    sessions and (b) the same build serving history + turn as fresh prompts through serve_fsm, today's only way;
                    three runs each in alternation (every (a) run on fresh sessions with a turn 1 of their own): new tok/s,
                    prefill_s, rows computed; how many of the 256 items' ids agree (the sessions' histories hold rows the
                    decode steps wrote, the fresh prompts recompute them on the prompt path: ids may part at a near tie).
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

SLOTS, CTX, REPS = 256, 2048, 3
STEP_LIMIT_S = {"attention": 300, "extend": 600, "serve": 900}


def spread(values):
    return {"median": round(float(np.median(values)), 4), "min_max": [round(float(min(values)), 4), round(float(max(values)), 4)]}


def step_attention():
    pkg = load_package()
    hip = pkg.hipabi.load(0)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle import orc
    orc.build(ref=False)
    oracle = orc.load_oracle()
    from helpers import Q4, Q8, act_rows, rng, row_bytes
    from test_block_rows_gpu import alloc_acts, make_block
    E, H, KVH, F = 2048, 32, 4, 5632
    r = rng(17)
    w, widths = make_block(hip, oracle, r, Q4, E, H, KVH, F, 0)
    g = np.random.default_rng(2026)
    rows = [int(x) for x in g.integers(32, 97, 32)]
    ctxs = [int(x) for x in g.integers(300, 1501, 32)]
    n = sum(rows)
    starts = [0] + [int(x) for x in np.cumsum(rows)]
    ints = dict(adtype=Q8, wdtype=Q4, n_embd=E, n_heads=H, n_kv_heads=KVH, n_ffn=F)
    bufs = dict(w)
    bufs.update(alloc_acts(hip, widths, n, 0, Q8))
    bufs["inp"] = hip.upload(act_rows(oracle, r, n, E, Q8)[0])
    # K / V rows to stand behind the segments: valid Q8 rows (what they hold does not change the launches' work)
    kv_rows = act_rows(oracle, r, 1500, KVH * (E // H), Q8)[0]
    rb = row_bytes(Q8, KVH * (E // H))
    assert kv_rows.shape == (1500, rb)
    sets = [(hip.upload(kv_rows), hip.upload(kv_rows)) for _ in range(32)]
    pre = (hip.upload(kv_rows[:1024]), hip.upload(kv_rows[:1024]))

    def continued():
        hip.set_row_segments(starts)
        hip.set_row_contexts([[(k, v, c) for (k, v), c in zip(sets, ctxs)]])
        assert hip.block_rows_continued(n, ints, bufs, 0)

    def prefixed():
        hip.set_row_segments(starts)
        assert hip.block_rows_prefixed(n, ints, bufs, pre[0], pre[1], 1024)

    def measure(fn, reps=20):
        fn()
        hip.sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        hip.sync()
        wall_us = 1e6 * (time.perf_counter() - t0) / reps
        out = {"block_wall_us": round(wall_us, 1), "rope_us": [], "attention_us": []}
        for _ in range(REPS):
            hip.prof_enable(True)
            fn()
            prof = hip.prof_read()
            hip.prof_enable(False)
            out["rope_us"].append(round(1e3 * prof.get("rotary_emb", (0, 0.0))[1], 1))
            out["attention_us"].append(round(1e3 * prof.get("qkv_attn_tiled", (0, 0.0))[1], 1))
        out["attention_launches"] = prof.get("qkv_attn_tiled", (0, 0.0))[0]
        return out

    res = {"segments": 32, "rows": n, "contexts": "300..1500", "context_rows_in_all": sum(ctxs), "prefix_rows": 1024,
           "continued": measure(continued), "prefixed_one_1024_row_prefix": measure(prefixed)}
    hip.set_row_contexts(None)
    hip.set_row_segments(None)
    return res


def step_extend():
    pkg = load_package()
    pkg.hipabi.load(0)
    host = pkg.load_host()
    cfg = host.default_config(4, 3)
    cfg.max_ctx = CTX
    b = host.batch(cfg, SLOTS)
    b.load_synthetic(4242)
    g = np.random.default_rng(2026)
    hist = [int(x) + 64 for x in g.integers(256, 513, SLOTS)]              # turn 1: the prompt and its 64 new ids
    turn = [int(x) for x in g.integers(32, 97, SLOTS)]
    ids = [[int(t) for t in host.synthetic_tokens(h + t, seed=3000 + q, n_vocab=cfg.n_vocab)] for q, (h, t) in enumerate(zip(hist, turn))]

    def calls(lengths, most=32, rows=4096):
        out, cur, tot = [], [], 0
        for q, n in enumerate(lengths):
            if cur and (len(cur) == most or tot + n > rows):
                out.append(cur)
                cur, tot = [], 0
            cur.append(q)
            tot += n
        out.append(cur)
        return out

    whole_calls = calls([h + t for h, t in zip(hist, turn)])
    hist_calls = calls(hist)
    turn_calls = calls(turn)

    def fresh(want=False):
        first = []
        for c in whole_calls:
            lg = b.prefill_many(c, [ids[q] for q in c], want=want)
            if want:
                first += np.argmax(lg, axis=1).tolist()
        return first

    def histories():
        for c in hist_calls:
            b.prefill_many(c, [ids[q][:hist[q]] for q in c], want=False)

    def extended():
        first = []
        for c in turn_calls:
            first += b.extend_many(c, [hist[q] for q in c], [ids[q][hist[q]:] for q in c], want=False)[1].tolist()
        return first

    res = {"sequences": SLOTS, "history_ids": "320..576", "turn_ids": "32..96", "turn_ids_in_all": sum(turn), "history_ids_in_all": sum(hist),
           "calls_fresh": len(whole_calls), "calls_extend": len(turn_calls), "runs": []}
    # warm-up (first-use allocations) and the comparison of the turns' first ids; the timed runs copy no logits back either way
    first_fresh = fresh(want=True)
    histories()
    res["same_first_ids"] = first_fresh == extended()
    for rep in range(REPS):
        for mode in ("fresh", "extend"):
            if mode == "extend":
                histories()                                                # (not timed: the state a first turn leaves)
            rows0 = b.prefix_info()[2]
            t0 = time.perf_counter()
            fresh() if mode == "fresh" else extended()
            wall = time.perf_counter() - t0
            res["runs"].append({"mode": mode, "rep": rep, "wall_s": round(wall, 4), "rows_computed": int(b.prefix_info()[2] - rows0),
                                "turn_ids_per_s": round(sum(turn) / wall, 1)})
    for mode in ("fresh", "extend"):
        r = [x for x in res["runs"] if x["mode"] == mode]
        res[mode] = {"wall_s": spread([x["wall_s"] for x in r]), "turn_ids_per_s": spread([x["turn_ids_per_s"] for x in r]), "rows_computed": r[0]["rows_computed"]}
    b.close()
    return res


def step_serve():
    pkg = load_package()
    pkg.hipabi.load(0)
    host = pkg.load_host()
    cfg = host.default_config(4, 3)
    cfg.max_ctx = CTX
    b = host.batch(cfg, SLOTS)
    b.load_synthetic(4242)
    g = np.random.default_rng(2026)
    p1 = [[int(t) for t in host.synthetic_tokens(int(n), seed=4000 + q, n_vocab=cfg.n_vocab)] for q, n in enumerate(g.integers(256, 513, SLOTS))]
    u2 = [[int(t) for t in host.synthetic_tokens(int(n), seed=5000 + q, n_vocab=cfg.n_vocab)] for q, n in enumerate(g.integers(32, 97, SLOTS))]
    b.sessions_reserve(SLOTS)
    res = {"slots": SLOTS, "sessions": SLOTS, "turn_1": "256..512 ids + 64 new", "turn_2": "32..96 ids + 64 new", "runs": []}

    def turn_one():
        ss = [b.session_open() for _ in range(SLOTS)]
        ids, _, _ = b.serve_sessions([(s, p) for s, p in zip(ss, p1)], CTX, -1, 1, 1.0, 7, slice_steps=8, max_new=64)
        return ss, ids

    ss, hist = turn_one()                                                  # warm-up, and the histories the fresh way is given
    whole = [h.tolist() + u for h, u in zip(hist, u2)]
    warm, _, _ = b.serve_sessions([(s, u) for s, u in zip(ss, u2)], CTX, -1, 1, 1.0, 7, slice_steps=8, max_new=64)
    b.serve_fsm(whole[:SLOTS], CTX, -1, 1, 1.0, 7, -1, slice_steps=8, max_new=4)
    for s in ss:
        b.session_close(s)
    got = {}
    for rep in range(REPS):
        for mode in ("fresh", "sessions"):
            if mode == "sessions":
                ss, again = turn_one()                                     # (not timed)
                assert all(np.array_equal(x, y) for x, y in zip(again, hist)), "turn 1 is repeatable"
                info0 = b.sessions_info()
            rows0 = b.prefix_info()[2]
            t0 = time.perf_counter()
            if mode == "fresh":
                ids, st, _ = b.serve_fsm(whole, CTX, -1, 1, 1.0, 7, -1, slice_steps=8, max_new=64)
            else:
                ids, st, _ = b.serve_sessions([(s, u) for s, u in zip(ss, u2)], CTX, -1, 1, 1.0, 7, slice_steps=8, max_new=64)
            wall = time.perf_counter() - t0
            run = {"mode": mode, "rep": rep, "new_tok_s": round(st["new_tokens"] / wall, 1), "wall_s": round(wall, 4), "prefill_s": round(st["prefill_s"], 4),
                   "decode_s": round(st["decode_s"], 4), "new_tokens": int(st["new_tokens"]), "rows_computed": int(b.prefix_info()[2] - rows0)}
            if mode == "sessions":
                info1 = b.sessions_info()
                run["session_rows_computed"], run["session_rows_kept"], run["turns_continued"] = int(info1[4] - info0[4]), int(info1[5] - info0[5]), int(info1[3] - info0[3])
                for s in ss:
                    b.session_close(s)
            res["runs"].append(run)
            got[mode] = ids
    res["items_with_equal_ids"] = int(sum(1 for x, y in zip(got["fresh"], got["sessions"]) if np.array_equal(x, y)))
    # (how far the two ways agree: the turn's first id is chosen from a row both ways compute on the prompt path, behind histories
    #  whose last 63 rows differ in origin; from there on the runs are greedy walks over near-flat synthetic logits)
    common = [int(np.argmin(np.append(x[len(w):len(w) + 64] == y[len(w):len(w) + 64], False))) for x, y, w in zip(got["fresh"], got["sessions"], whole)]
    res["items_with_equal_first_new_id"] = int(sum(1 for c in common if c >= 1))
    res["new_ids_in_common_before_the_first_difference"] = {"median": float(np.median(common)), "min": int(min(common)), "max": int(max(common))}
    res["kv_bytes_per_session"] = int(b.sessions_info()[1])
    for mode in ("fresh", "sessions"):
        r = [x for x in res["runs"] if x["mode"] == mode]
        res[mode] = {"new_tok_s": spread([x["new_tok_s"] for x in r]), "prefill_s": spread([x["prefill_s"] for x in r]), "wall_s": spread([x["wall_s"] for x in r]),
                     "rows_computed": r[0]["rows_computed"]}
    b.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S), default=None)
    a = ap.parse_args()
    if a.step:
        print(json.dumps({"attention": step_attention, "extend": step_extend, "serve": step_serve}[a.step]()))
        return 0
    res = {"what": "continued prompt rows, TinyLlama-1.1B q4 synthetic: a second turn of 32..96 ids behind 320..576 ids, %d sequences" % SLOTS}
    for step in ("attention", "extend", "serve"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step]
        p = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT_S[step])] + cmd, capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            sys.stderr.write("\nsessions_cost: step %s ended with %d: stopping\n" % (step, p.returncode))
            return 1
        res[step] = json.loads(p.stdout.strip().splitlines()[-1])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
