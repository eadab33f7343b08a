#!/usr/bin/env python3
"""The cost of bias tables on the device, one JSON line on stdout
(tools/bias_cost.py [--out profiles/bias_cost.json]).

Full-size TinyLlama, q4 weights, synthetic.  For 1, 64 and 256 sequences: ms per sampled decode step (k 40, T 0.9) over the
steps that end at n = CTX, measured as tools/sampler_cost.py does (generation from prompts of CTX - STEPS ids timed up to CTX
ids and up to one new id, the difference divided by the STEPS - 1 decode steps between them: the prompt and the first id
cancel), in three states of the same decoder:
  parent    no table was ever bound: the step ends in k_dec_sample.  This is the same build, not a build of the commit before
            bias tables existed; it stands for that commit's sampled step because k_dec_sample's gfx950 code is identical to
            it, instruction for instruction, and nothing else of the step changed;
  no_table  a table was bound once and cleared again: the step ends in k_dec_sample_b, every sequence on its unbiased branch;
  bound     every sequence draws under a table (fill 0, a few ids banned).
`spread` is the largest difference between two repeats of the same state: what a difference between states has to exceed
to mean anything.  And the sampler launch alone on one real logits row (in-library profiler), without and with a bias row."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

CTX, K, TEMP, SEED = 512, 40, 0.9, 7
BANNED = [(2, float("-inf")), (1, float("-inf")), (13, float("-inf"))]


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
    res = {"what": f"bias table cost, TinyLlama-1.1B q4 synthetic, ctx {CTX}, k 40, T 0.9", "steps": a.steps, "ms_per_step": {}}
    P = CTX - a.steps

    def states(obj, sampled, biased, bind_once):
        out = {}
        for name, gen in (("parent", sampled), ("no_table", sampled), ("bound", biased)):
            if name == "no_table":
                bind_once()
            ms, spread = step_ms(gen, a.steps)
            out[name] = round(ms, 4)
            out[name + "_spread"] = round(spread, 4)
        out["no_table_over_parent"] = round(out["no_table"] / out["parent"], 4)
        out["bound_over_parent"] = round(out["bound"] / out["parent"], 4)
        return out

    m = host.model(cfg)
    m.load_synthetic(4242)
    m.set_bias_table(0, BANNED)
    prompt = list(host.synthetic_tokens(P, seed=3, n_vocab=cfg.n_vocab))

    def bind_once_model():
        assert m.set_seq_bias_rc(0) == 0 and m.set_seq_bias_rc(-1) == 0

    res["ms_per_step"]["1"] = states(m, lambda mt: m.generate_topk(prompt, mt, -1, K, TEMP, SEED),
                                     lambda mt: m.generate_biased(prompt, mt, -1, K, TEMP, SEED, 0, 0), bind_once_model)
    # the sampler launch on one logits row of the model, without and with a bias row
    import numpy as np
    row = m.logits(prompt, 0)
    buf = pkg.hipabi.DeviceBuffer.from_numpy(hip, row[None, :])
    bias = np.zeros(cfg.n_vocab, np.float32)
    for j, v in BANNED:
        bias[j] = v
    bbuf = pkg.hipabi.DeviceBuffer.from_numpy(hip, bias[None, :])
    for name, call in (("decode_sample_us", lambda i: hip.sample_rows(buf, 1, cfg.n_vocab, 0, K, TEMP, SEED, 0, P + i)),
                       ("decode_sample_biased_us", lambda i: hip.sample_rows_biased(buf, bbuf, 1, cfg.n_vocab, 0, 0, K, TEMP, SEED, 0, P + i))):
        call(0)
        hip.prof_enable(True)
        n0, ms0 = hip.prof_read().get("decode_sample", (0, 0.0))     # (whatever the profiler already holds)
        for i in range(200):
            call(i)
        n, ms = hip.prof_read()["decode_sample"]
        hip.prof_enable(False)
        res[name] = round(1e3 * (ms - ms0) / (n - n0), 2)
    m.close()
    for S in (64, 256):
        b = host.batch(cfg, S)
        b.load_synthetic(4242)
        b.set_bias_table(0, BANNED)
        prompts = [list(host.synthetic_tokens(P, seed=10 + q, n_vocab=cfg.n_vocab)) for q in range(S)]

        def bind_once_batch():
            b.set_seq_bias(0, 0)
            b.set_seq_bias(0, -1)

        res["ms_per_step"][str(S)] = states(b, lambda mt: b.generate_topk(prompts, mt, -1, K, TEMP, SEED),
                                            lambda mt: b.generate_biased(prompts, mt, -1, K, TEMP, SEED, None, 0, 0), bind_once_batch)
        b.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
