#!/usr/bin/env python3
"""The cost of Mirostat v2 on the device, one JSON line on stdout
(tools/mirostat_cost.py [--parent-root DIR] [--out profiles/mirostat_cost.json]), in the manner of tools/nucleus_cost.py.

Full-size TinyLlama, q4 weights, synthetic.  For 1, 64 and 256 sequences: ms per sampled decode step (T 0.9) over the steps that
end at n = CTX (generation from prompts of CTX - STEPS ids timed up to CTX ids and up to one new id, the difference divided by the
STEPS - 1 decode steps between them: the prompt and the first id cancel), three repeats each (the best, and `spread` = the largest
difference between two repeats), in four states:
  parent     the PARENT COMMIT'S BUILD: a checkout of the commit before this feature, built, at --parent-root; measured by a
             child process that loads that tree's package (this script with --child-root).  Left out when no root is given;
  unbound    this build, k 40, no sequence has ever been bound: the step ends in k_dec_sample, as the parent's does;
  miro40     k 40 under Mirostat (tau 5, eta 0.1) on every sequence: the step ends in k_dec_sample_miro;
  miro_full  k = n_vocab under the same request on every sequence.
And the sampler launch alone on one real logits row (in-library profiler): the plain draw and the cut draw at k 40 and at
k = n_vocab, and the Mirostat draw at both.  Nothing here is a threshold."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CTX, K, TEMP, SEED, TOP_P, MIN_P, TAU, ETA = 512, 40, 0.9, 7, 0.9, 0.05, 5.0, 0.1
WIDTHS = (1, 64, 256)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def step_ms(gen, steps, repeats=3):
    """(ms per step of gen(max_tokens) over the last `steps` steps before CTX, spread of the repeats)"""
    gen(CTX - steps + 1)                                      # warm: graphs captured, prompt path compiled
    got = []
    for _ in range(repeats):
        t_all = timed(lambda: gen(CTX))
        t_one = timed(lambda: gen(CTX - steps + 1))
        got.append(1e3 * (t_all - t_one) / (steps - 1))
    return min(got), max(got) - min(got)


def measure(root, steps, cut):
    """{width: {state: ms, state_spread: ms}} with the package of the tree at `root`; cut: also the Mirostat states and the launches"""
    sys.path.insert(0, root)
    from __graft_entry__ import load_package
    pkg = load_package()
    hip = pkg.hipabi.load(0)
    host = pkg.load_host()
    cfg = host.default_config(4, 3)
    cfg.max_ctx = CTX
    P, V = CTX - steps, cfg.n_vocab
    res, extra = {}, {}
    for S in WIDTHS:
        o = host.model(cfg) if S == 1 else host.batch(cfg, S)
        o.load_synthetic(4242)
        prompts = [list(host.synthetic_tokens(P, seed=(3 if S == 1 else 10 + q), n_vocab=V)) for q in range(S)]
        who = prompts[0] if S == 1 else prompts
        states = [("unbound", lambda mt: o.generate_topk(who, mt, -1, K, TEMP, SEED))]
        if cut:
            # (unbound is measured first: afterwards the decoder has had a sequence bound and launches k_dec_sample_miro)
            states += [("miro40", lambda mt: o.generate_mirostat(who, mt, TAU, ETA, -1, K, TEMP, SEED)),
                       ("miro_full", lambda mt: o.generate_mirostat(who, mt, TAU, ETA, -1, V, TEMP, SEED))]
        out = {}
        for name, gen in states:
            ms, spread = step_ms(gen, steps)
            out[name] = round(ms, 4)
            out[name + "_spread"] = round(spread, 4)
        res[str(S)] = out
        if S == 1 and cut:
            row = o.logits(prompts[0], 0)
            buf = pkg.hipabi.DeviceBuffer.from_numpy(hip, row[None, :])
            for name, call in (("draw_k40_us", lambda i: hip.sample_rows(buf, 1, V, 0, K, TEMP, SEED, 0, P + i)),
                               ("draw_full_us", lambda i: hip.sample_rows(buf, 1, V, 0, V, TEMP, SEED, 0, P + i)),
                               ("cut_k40_us", lambda i: hip.sample_rows_cut(buf, 1, V, 0, K, TEMP, SEED, 0, P + i, TOP_P, MIN_P, info=False)),
                               ("cut_full_us", lambda i: hip.sample_rows_cut(buf, 1, V, 0, V, TEMP, SEED, 0, P + i, TOP_P, MIN_P, info=False)),
                               ("miro_k40_us", lambda i: hip.sample_rows_miro(buf, 1, V, 0, K, TEMP, SEED, 0, P + i, 10 << 16, TAU, ETA, info=False)),
                               ("miro_full_us", lambda i: hip.sample_rows_miro(buf, 1, V, 0, V, TEMP, SEED, 0, P + i, 10 << 16, TAU, ETA, info=False))):
                call(0)
                hip.prof_enable(True)
                n0, ms0 = hip.prof_read().get("decode_sample", (0, 0.0))     # (whatever the profiler already holds)
                for i in range(200):
                    call(i)
                n, ms = hip.prof_read()["decode_sample"]
                hip.prof_enable(False)
                extra[name] = round(1e3 * (ms - ms0) / (n - n0), 2)
            _, _, info = hip.sample_rows_miro(buf, 1, V, 0, V, TEMP, SEED, 0, P, 10 << 16, TAU, ETA)
            extra["full_row_n_keep"] = int(info["n_keep"][0])
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
        res, _ = measure(a.child_root, a.steps, cut=False)
        print(json.dumps(res))
        return
    res = {"what": f"Mirostat v2 cost, TinyLlama-1.1B q4 synthetic, ctx {CTX}, T {TEMP}, tau {TAU}, eta {ETA}", "steps": a.steps, "ms_per_step": {}}
    parent = None
    if a.parent_root:
        # (a fresh child process, before this one opens the GPU)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-root", os.path.abspath(a.parent_root), "--steps", str(a.steps)],
                           capture_output=True, text=True, timeout=1500)
        if r.returncode != 0:
            raise SystemExit("the parent's measurement failed:\n" + r.stderr[-2000:])
        parent = json.loads(r.stdout.strip().splitlines()[-1])
    own, extra = measure(ROOT, a.steps, cut=True)
    for S in map(str, WIDTHS):
        out = {}
        if parent:
            out["parent"], out["parent_spread"] = parent[S]["unbound"], parent[S]["unbound_spread"]
        out.update(own[S])
        if parent:
            out["unbound_over_parent"] = round(out["unbound"] / out["parent"], 4)
        out["miro40_over_unbound"] = round(out["miro40"] / out["unbound"], 4)
        out["miro_full_over_unbound"] = round(out["miro_full"] / out["unbound"], 4)
        res["ms_per_step"][S] = out
    res.update(extra)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
