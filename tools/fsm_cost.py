#!/usr/bin/env python3
"""The cost of token automata on the device, one JSON line on stdout
(tools/fsm_cost.py [--parent-root DIR] [--out profiles/fsm_cost.json]).

Full-size TinyLlama, q4 weights, synthetic.  For 1, 64 and 256 sequences: ms per sampled decode step (k 40, T 0.9) over the steps
that end at n = CTX, measured as tools/penalty_cost.py does (generation from prompts of CTX - STEPS ids timed up to CTX ids and up to
one new id, the difference divided by the STEPS - 1 decode steps between them: the prompt and the first id cancel), three repeats
each (the best, and `spread` = the largest difference between two repeats), in four states:
  parent    the PARENT COMMIT'S BUILD: a checkout of the commit before this feature, built, at --parent-root; measured by a
            child process that loads that tree's package (this script with --child-root).  Left out when no root is given;
  no_fsm    this build, no sequence has ever been bound: the step ends in k_dec_sample, as the parent's does;
  stop      a stop pool (Aho-Corasick over four sequences that do not occur) on every sequence: k_dec_sample_fsm, nothing banned;
  mask      a pool of 256 live states that each allow a quarter of the ids, every sequence started in a state of its own: every
            sequence reads another 64 KB row of `next` per step, beside its logits row.
A bound run in which a sequence ended early would time fewer steps: the script refuses to report it.
And the sampler launch alone on real logits rows (in-library profiler), 1 / 64 / 256 rows per launch, every row in a state of its
own: the penalised launch (gten_hip_sample_rows_pen, window 512, cut (0.9, 0.05)) against the same under the mask
(gten_hip_sample_rows_fsm), and the two without a penalty (gten_hip_sample_rows_cut against the masked launch).  Nothing here is a
threshold."""
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
MASK_STATES, DENSITY = 256, 0.25


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


def mask_pool(V):
    """MASK_STATES live states, each allowing about DENSITY of the ids and leading anywhere in the pool"""
    g = np.random.default_rng(5)
    nxt = g.integers(0, MASK_STATES, (MASK_STATES, V)).astype(np.uint16)
    nxt[g.random((MASK_STATES, V)) >= DENSITY] = 0xFFFF
    return nxt, np.zeros(MASK_STATES, np.uint8)


def measure(root, steps, fsm):
    """{width: {state: ms, state_spread: ms}} with the package of the tree at `root`; fsm: also the bound states and the launches"""
    sys.path.insert(0, root)
    from __graft_entry__ import load_package
    pkg = load_package()
    hip = pkg.hipabi.load(0)
    host = pkg.load_host()
    res, extra = {}, {}
    for S in WIDTHS:
        cfg = host.default_config(4, 3)
        cfg.max_ctx = CTX
        P, V = CTX - steps, cfg.n_vocab
        o = host.model(cfg) if S == 1 else host.batch(cfg, S)
        o.load_synthetic(4242)
        prompts = [list(host.synthetic_tokens(P, seed=(3 if S == 1 else 10 + q), n_vocab=V)) for q in range(S)]
        who = prompts[0] if S == 1 else prompts
        out = res.setdefault(str(S), {})

        def run(name, gen):
            ms, spread = step_ms(gen, CTX, steps)
            out[name] = round(ms, 4)
            out[name + "_spread"] = round(spread, 4)

        # (no_fsm is measured first: afterwards the decoder has had a sequence bound and launches k_dec_sample_fsm)
        run("no_fsm", lambda mt: o.generate_topk(who, mt, -1, K, TEMP, SEED))
        if fsm:
            def bound(start):
                def gen(mt):
                    ids, ended = o.generate_fsm(who, mt, start if S == 1 else np.asarray(start, np.int32), -1, K, TEMP, SEED)
                    if np.any(np.asarray(ended) != 0):
                        raise SystemExit("a bound sequence ended early: the timing would be of fewer steps")
                return gen
            stops = pkg.hostabi.Fsm(host, V)
            s0 = stops.add_stop([[V - 1] * 4, [V - 2, V - 3, V - 2, V - 3], [5, 5, 5, 5, 5], [V - 7, 7, V - 7]])
            o.set_fsm(stops)
            run("stop", bound(s0 if S == 1 else [s0] * S))
            nxt, flags = mask_pool(V)
            masks = pkg.hostabi.Fsm(host, V)
            m0 = masks.add_table(nxt, flags)
            o.set_fsm(masks)
            run("mask", bound(m0 + 1 if S == 1 else [m0 + q % MASK_STATES for q in range(S)]))
            if S == 1:
                row = o.logits(prompts[0], 0)
                g = np.random.default_rng(1)
                pool = hip.fsm_upload(nxt, flags)
                for R in WIDTHS:
                    buf = pkg.hipabi.DeviceBuffer.from_numpy(hip, np.ascontiguousarray(np.tile(row, (R, 1)) + g.standard_normal((R, V)).astype(np.float32)))
                    st, states = np.arange(R, dtype=np.uint32), np.arange(R, dtype=np.int32) % MASK_STATES
                    h512 = [g.integers(0, V, 512) for _ in range(R)]
                    for name, call in (("cut_k40", lambda i: hip.sample_rows_cut(buf, R, V, V, K, TEMP, SEED, st, P + i, TOP_P, MIN_P, info=False)),
                                       ("fsm_cut_k40", lambda i: hip.sample_rows_fsm(buf, R, V, V, pool, states, K, TEMP, SEED, st, P + i, top_p=TOP_P, min_p=MIN_P)),
                                       ("pen_cut_k40_h512", lambda i: hip.sample_rows_pen(buf, R, V, V, K, TEMP, SEED, st, P + i, h512, *PEN, TOP_P, MIN_P)),
                                       ("fsm_pen_cut_k40_h512", lambda i: hip.sample_rows_fsm(buf, R, V, V, pool, states, K, TEMP, SEED, st, P + i, h512, *PEN, TOP_P, MIN_P)),
                                       ("draw_k40", lambda i: hip.sample_rows(buf, R, V, V, K, TEMP, SEED, st, P + i)),
                                       ("fsm_draw_k40", lambda i: hip.sample_rows_fsm(buf, R, V, V, pool, states, K, TEMP, SEED, st, P + i))):
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
        res, _ = measure(a.child_root, a.steps, fsm=False)
        print(json.dumps(res))
        return
    res = {"what": f"token automaton cost, TinyLlama-1.1B q4 synthetic, ctx {CTX}, k {K}, T {TEMP}; mask: {MASK_STATES} states, density {DENSITY}",
           "steps": a.steps, "ms_per_step": {}}
    parent = None
    if a.parent_root:
        # (a fresh child process, before this one opens the GPU)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-root", os.path.abspath(a.parent_root), "--steps", str(a.steps)],
                           capture_output=True, text=True, timeout=1500)
        if r.returncode != 0:
            raise SystemExit("the parent's measurement failed:\n" + r.stderr[-2000:])
        parent = json.loads(r.stdout.strip().splitlines()[-1])
    own, extra = measure(ROOT, a.steps, fsm=True)
    for S in map(str, WIDTHS):
        out = {}
        if parent:
            out["parent"], out["parent_spread"] = parent[S]["no_fsm"], parent[S]["no_fsm_spread"]
        out.update(own[S])
        if parent:
            out["no_fsm_over_parent"] = round(out["no_fsm"] / out["parent"], 4)
        out["stop_over_no_fsm"] = round(out["stop"] / out["no_fsm"], 4)
        out["mask_over_no_fsm"] = round(out["mask"] / out["no_fsm"], 4)
        res["ms_per_step"][S] = out
    res.update(extra)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
