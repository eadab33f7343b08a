#!/usr/bin/env python3
"""The cost of binding a decoder to a regular expression, one JSON line on stdout
(tools/regex_cost.py [--out profiles/regex_cost.json] [--repeats 5]).

For byte automata of about 16, 256 and 4096 states over the vendored 32 003-id vocabulary (tests/golden/tokenizer.bin), the time from
"pattern in hand" to "pool adopted by the decoder" by two routes, on the same machine in the same run, on a small synthetic model with
that vocabulary:
  device   compile the pattern (Fsm.add_regex) and set the pool (gten_hip_decoder_set_fsm_parts: the byte automaton is uploaded, expanded
           over the vocabulary by k_fsm_expand and checked by k_fsm_check on the device);
  table    the only route there was before: compile, expand on the host (this library's own host expansion, plain C++ on one thread --
           a caller without it would write the same loop), hand the table to add_table, and gten_hip_decoder_set_fsm with its host check
           and its upload of the whole table.
Each with its parts, `repeats` times: the best, the median and the spread (largest minus smallest).  The vocabulary's byte strings
are made once, outside both.  Alongside, the expansion's launches alone (k_fsm_expand_flags + k_fsm_expand, the in-library profiler's
events) into a pool that exists, and the store bandwidth that is: rows x n_vocab x 2 bytes over that time.  Nothing here is a threshold."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(ROOT, "tests", "golden", "tokenizer.bin")
EOS = 2
PATTERNS = [("16", r"-?[0-9]{1,14}"), ("256", r"[A-Za-z]{1,255}"), ("4096", r"([a-z]{1,255} ){16}")]


def stats(xs):
    return {"best": round(min(xs), 3), "median": round(statistics.median(xs), 3), "spread": round(max(xs) - min(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    pkg = load_package()
    hip = pkg.hipabi.load(0)
    host = pkg.load_host()
    cfg = host.default_config(4, 3)
    cfg.max_ctx, cfg.n_embd, cfg.n_ffn, cfg.n_layers, cfg.n_heads, cfg.n_kv_heads = 64, 256, 512, 2, 4, 2
    V = cfg.n_vocab
    m = host.model(cfg)
    m.load_synthetic(4242)
    tok = host.tokenizer(VOCAB)
    vocab = tok.vocab_bytes(V)
    res = {"what": f"regular expression to adopted pool, {V} ids, {len(vocab[0])} vocabulary bytes; ms; {a.repeats} repeats", "sizes": {}}
    ms = lambda t0: 1e3 * (time.perf_counter() - t0)          # noqa: E731
    for name, pattern in PATTERNS:
        n256, acc = pkg.hostabi.byte_dfa(host, pattern)
        rows = len(acc) + 1
        out = {"pattern": pattern, "byte_states": len(acc), "pool_states": rows, "pool_mb": round(rows * V * 2 / 1e6, 1)}
        dev = {"compile": [], "set_fsm_parts": [], "total": []}
        tab = {"compile": [], "host_expand": [], "add_table": [], "set_fsm": [], "total": []}
        for r in range(a.repeats + 1):                        # (the first round of each route warms allocators and code: left out)
            t0 = time.perf_counter()
            f = pkg.hostabi.Fsm(host, V)
            f.set_vocab(vocab)
            f.add_regex(pattern, EOS)
            t1 = ms(t0)
            m.set_fsm(f)
            t2 = ms(t0)
            if r:
                dev["compile"].append(t1), dev["set_fsm_parts"].append(t2 - t1), dev["total"].append(t2)
            f.close()
            t0 = time.perf_counter()
            f = pkg.hostabi.Fsm(host, V)
            f.set_vocab(vocab)
            f.add_regex(pattern, EOS)
            t1 = ms(t0)
            nxt, flags = f.tables()
            t2 = ms(t0)
            g = pkg.hostabi.Fsm(host, V)
            g.add_table(nxt, flags)
            t3 = ms(t0)
            m.set_fsm(g)
            t4 = ms(t0)
            if r:
                tab["compile"].append(t1), tab["host_expand"].append(t2 - t1), tab["add_table"].append(t3 - t2), tab["set_fsm"].append(t4 - t3)
                tab["total"].append(t4)
            f.close()
            g.close()
            del nxt
        out["device_route_ms"] = {k: stats(v) for k, v in dev.items()}
        out["table_route_ms"] = {k: stats(v) for k, v in tab.items()}
        out["table_over_device"] = round(statistics.median(tab["total"]) / statistics.median(dev["total"]), 2)
        # the expansion's launches alone, into a pool that exists
        pool = (hip.alloc(rows * V * 2), hip.alloc(rows + 4), rows)
        hip.fsm_expand(pool, V, 0, vocab, n256, acc, EOS)
        launch = []
        for _ in range(a.repeats):
            hip.prof_enable(True)
            n0, ms0 = hip.prof_read().get("decode_sample", (0, 0.0))
            hip.fsm_expand(pool, V, 0, vocab, n256, acc, EOS)
            n, ms1 = hip.prof_read()["decode_sample"]
            hip.prof_enable(False)
            assert n - n0 == 2
            launch.append(ms1 - ms0)
        out["expand_launch_ms"] = stats(launch)
        out["expand_store_gb_s"] = round(rows * V * 2 / 1e9 / (statistics.median(launch) / 1e3), 1)
        assert hip.fsm_check_dev(pool, V) == (0, -1)
        pool[0].free()
        pool[1].free()
        res["sizes"][name] = out
    m.set_fsm(None)
    m.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
