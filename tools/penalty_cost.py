#!/usr/bin/env python3
"""The cost of repetition / frequency / presence penalties on the device, one JSON line on stdout
(tools/penalty_cost.py [--parent-root DIR] [--out profiles/penalty_cost.json]).

Full-size TinyLlama, q4 weights, synthetic.  For 1, 64 and 256 sequences: ms per sampled decode step (k 40, T 0.9) over the steps
that end at n = CTX, measured as tools/nucleus_cost.py does (generation from prompts of CTX - STEPS ids timed up to CTX ids and up to
one new id, the difference divided by the STEPS - 1 decode steps between them: the prompt and the first id cancel), three repeats
each (the best, and `spread` = the largest difference between two repeats), in three states:
  parent    the PARENT COMMIT'S BUILD: a checkout of the commit before this feature, built, at --parent-root; measured by a
            child process that loads that tree's package (this script with --child-root).  Left out when no root is given;
  no_pen    this build, no sequence has ever set a penalty: the step ends in k_dec_sample, as the parent's does;
  pen       (1.1, 0.1, 0.1) over the whole context (about CTX ids) on every sequence: the step ends in k_dec_sample_pen.
For one sequence also `pen_ctx2048`: the same at a context of 2048 ids (the history of 2048), beside `no_pen_ctx2048`.
And the sampler launch alone on real logits rows (in-library profiler), 1 / 64 / 256 rows per launch: the cut launch at k 40
(gten_hip_sample_rows_cut, (0.9, 0.05)) against the penalised launch (gten_hip_sample_rows_pen: the same row routine as
k_dec_sample_pen's, same cut) with windows of 512 and of 2048 ids, and the penalised plain draw.  Nothing here is a threshold."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CTX, K, TEMP, SEED, TOP_P, MIN_P = 512, 40, 0.9, 7, 0.9, 0.05
PEN = (1.1, 0.1, 0.1)
WIDTHS = (1, 64, 256)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def step_ms(gen, ctx, steps, repeats=3):
    """(ms per step of gen(max_tokens) over the last `steps` steps before ctx, spread of the repeats)"""
    gen(ctx - steps + 1)                                      # warm: graphs captured, prompt path compiled
    got = []
    for _ in range(repeats):
        t_all = timed(lambda: gen(ctx))
        t_one = timed(lambda: gen(ctx - steps + 1))
        got.append(1e3 * (t_all - t_one) / (steps - 1))
    return min(got), max(got) - min(got)


def measure(root, steps, pen):
    """{width: {state: ms, state_spread: ms}} with the package of the tree at `root`; pen: also the penalised states and the launches"""
    sys.path.insert(0, root)
    from __graft_entry__ import load_package
    pkg = load_package()
    hip = pkg.hipabi.load(0)
    host = pkg.load_host()
    res, extra = {}, {}
    for S in WIDTHS:
        for ctx in ((CTX, 2048) if S == 1 and pen else (CTX,)):
            cfg = host.default_config(4, 3)
            cfg.max_ctx = ctx
            P, V = ctx - steps, cfg.n_vocab
            o = host.model(cfg) if S == 1 else host.batch(cfg, S)
            o.load_synthetic(4242)
            prompts = [list(host.synthetic_tokens(P, seed=(3 if S == 1 else 10 + q), n_vocab=V)) for q in range(S)]
            who = prompts[0] if S == 1 else prompts
            tag = "" if ctx == CTX else f"_ctx{ctx}"
            states = [("no_pen" + tag, lambda mt: o.generate_topk(who, mt, -1, K, TEMP, SEED))]
            if pen:
                # (no_pen is measured first: afterwards the decoder has had a penalty set and launches k_dec_sample_pen)
                states += [("pen" + tag, lambda mt: o.generate_penalized(who, mt, -1, K, TEMP, SEED, rep=PEN[0], freq=PEN[1], pres=PEN[2]))]
            out = res.setdefault(str(S), {})
            for name, gen in states:
                ms, spread = step_ms(gen, ctx, steps)
                out[name] = round(ms, 4)
                out[name + "_spread"] = round(spread, 4)
            if S == 1 and pen and ctx == CTX:
                row = o.logits(prompts[0], 0)
                g = np.random.default_rng(1)
                for R in WIDTHS:
                    buf = pkg.hipabi.DeviceBuffer.from_numpy(hip, np.ascontiguousarray(np.tile(row, (R, 1)) + g.standard_normal((R, V)).astype(np.float32)))
                    st = np.arange(R, dtype=np.uint32)
                    h512, h2048 = [g.integers(0, V, 512) for _ in range(R)], [g.integers(0, V, 2048) for _ in range(R)]
                    for name, call in (("cut_k40", lambda i: hip.sample_rows_cut(buf, R, V, V, K, TEMP, SEED, st, P + i, TOP_P, MIN_P, info=False)),
                                       ("pen_cut_k40_h512", lambda i: hip.sample_rows_pen(buf, R, V, V, K, TEMP, SEED, st, P + i, h512, *PEN, TOP_P, MIN_P)),
                                       ("pen_cut_k40_h2048", lambda i: hip.sample_rows_pen(buf, R, V, V, K, TEMP, SEED, st, P + i, h2048, *PEN, TOP_P, MIN_P)),
                                       ("draw_k40", lambda i: hip.sample_rows(buf, R, V, V, K, TEMP, SEED, st, P + i)),
                                       ("pen_draw_k40_h512", lambda i: hip.sample_rows_pen(buf, R, V, V, K, TEMP, SEED, st, P + i, h512, *PEN)),
                                       ("pen_draw_k40_h2048", lambda i: hip.sample_rows_pen(buf, R, V, V, K, TEMP, SEED, st, P + i, h2048, *PEN))):
                        call(0)
                        hip.prof_enable(True)
                        n0, ms0 = hip.prof_read().get("decode_sample", (0, 0.0))     # (whatever the profiler already holds)
                        for i in range(100):
                            call(i)
                        n, ms = hip.prof_read()["decode_sample"]
                        hip.prof_enable(False)
                        extra.setdefault(f"launch_us_{R}_rows", {})[name] = round(1e3 * (ms - ms0) / (n - n0), 2)
            o.close()
    return res, extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--child-root", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_root:
        res, _ = measure(a.child_root, a.steps, pen=False)
        print(json.dumps(res))
        return
    res = {"what": f"penalty cost, TinyLlama-1.1B q4 synthetic, ctx {CTX}, k {K}, T {TEMP}, (r, freq, pres) {PEN}", "steps": a.steps, "ms_per_step": {}}
    parent = None
    if a.parent_root:
        # (a fresh child process, before this one opens the GPU)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-root", os.path.abspath(a.parent_root), "--steps", str(a.steps)],
                           capture_output=True, text=True, timeout=1500)
        if r.returncode != 0:
            raise SystemExit("the parent's measurement failed:\n" + r.stderr[-2000:])
        parent = json.loads(r.stdout.strip().splitlines()[-1])
    own, extra = measure(ROOT, a.steps, pen=True)
    for S in map(str, WIDTHS):
        out = {}
        if parent:
            out["parent"], out["parent_spread"] = parent[S]["no_pen"], parent[S]["no_pen_spread"]
        out.update(own[S])
        if parent:
            out["no_pen_over_parent"] = round(out["no_pen"] / out["parent"], 4)
        out["pen_over_no_pen"] = round(out["pen"] / out["no_pen"], 4)
        res["ms_per_step"][S] = out
    res.update(extra)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
