#!/usr/bin/env python3
"""The cost of top-k sampling on the device, one JSON line on stdout
(tools/sampler_cost.py [--out profiles/sampler_cost.json]).

Full-size TinyLlama, q4 weights, synthetic.  For 1, 64 and 256 sequences: ms per decode step, greedy against sampled
(k 40, T 0.9), over the steps that end at n = 2048 -- generation from prompts of 2048 - STEPS ids timed with STEPS + 1
ids and with 1 id, the difference divided by STEPS (the prompt and the first id cancel).  The sampler launch's own time
(HIP events of the in-library profiler around gten_hip_sample_rows on one real logits row).  And the host loop the
command line used to run -- one step, its logits copied to the host and a top-k draw there, per token -- against the
device path's tok/s."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

CTX, K, TEMP, SEED = 2048, 40, 0.9, 7


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def step_ms(gen, steps):
    """ms per step of gen(max_tokens) over the last `steps` steps before CTX"""
    gen(CTX - steps + 1)                                      # warm: graphs captured, prompt path compiled
    t_all = min(timed(lambda: gen(CTX + 1 - 1)) for _ in range(2))
    t_one = min(timed(lambda: gen(CTX - steps + 1)) for _ in range(2))
    return 1e3 * (t_all - t_one) / (steps - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=128)
    a = ap.parse_args()
    pkg = load_package()
    hip = pkg.hipabi.load(0)
    host = pkg.load_host()
    cfg = host.default_config(4, 3)
    cfg.max_ctx = CTX
    res = {"what": "sampler cost, TinyLlama-1.1B q4 synthetic, ctx 2048, k 40, T 0.9", "steps": a.steps, "ms_per_step": {}}
    P = CTX - a.steps
    m = host.model(cfg)
    m.load_synthetic(4242)
    prompt = list(host.synthetic_tokens(P, seed=3, n_vocab=cfg.n_vocab))
    g = step_ms(lambda mt: m.generate(prompt, mt), a.steps)
    s = step_ms(lambda mt: m.generate_topk(prompt, mt, -1, K, TEMP, SEED), a.steps)
    res["ms_per_step"]["1"] = {"greedy": round(g, 4), "sampled": round(s, 4), "ratio": round(s / g, 4)}
    # the sampler launch on one logits row of the model
    row = m.logits(prompt, 0)
    buf = pkg.hipabi.DeviceBuffer.from_numpy(hip, row[None, :])
    hip.sample_rows(buf, 1, cfg.n_vocab, 0, K, TEMP, SEED, 0, P)
    hip.prof_enable(True)
    for i in range(200):
        hip.sample_rows(buf, 1, cfg.n_vocab, 0, K, TEMP, SEED, 0, P + i)
    prof = hip.prof_read()
    hip.prof_enable(False)
    n, ms = prof["decode_sample"]
    res["decode_sample_us"] = round(1e3 * ms / n, 2)
    # the old host loop: a step, 128 KB of logits to the host, a top-k draw there, per token
    rng = np.random.default_rng(0)
    n_host = 64
    ids = list(prompt)
    m.logits(ids, 0, want=False)

    def host_loop():
        for _ in range(n_host):
            x = m.logits(ids, len(ids) - 1).astype(np.float64) / TEMP
            c = np.argpartition(-x, K)[:K]
            w = np.exp(x[c] - x[c].max())
            ids.append(int(c[rng.choice(K, p=w / w.sum())]))
    t = timed(host_loop)
    res["host_loop_tok_s"] = round(n_host / t, 1)
    res["device_sampled_tok_s"] = round(1e3 / s, 1)
    m.close()
    for S in (64, 256):
        b = host.batch(cfg, S)
        b.load_synthetic(4242)
        prompts = [list(host.synthetic_tokens(P, seed=10 + q, n_vocab=cfg.n_vocab)) for q in range(S)]
        g = step_ms(lambda mt: b.generate(prompts, mt), a.steps)
        s = step_ms(lambda mt: b.generate_topk(prompts, mt, -1, K, TEMP, SEED), a.steps)
        res["ms_per_step"][str(S)] = {"greedy": round(g, 4), "sampled": round(s, 4), "ratio": round(s / g, 4)}
        b.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
