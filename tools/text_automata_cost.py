#!/usr/bin/env python3
"""The cost of stop strings given as text and of JSON schemas, one JSON line on stdout
(tools/text_automata_cost.py [--out profiles/text_automata_cost.json] [--repeats 5] [--root CHECKOUT] [--unbound-only]).

1. For 1, 16 and 256 stop strings of 8 bytes over the vendored 32 003-id vocabulary (tests/golden/tokenizer.bin), the time from "strings
   in hand" to "pool adopted by the decoder" by two routes, on a small synthetic model with that vocabulary:
     device   Fsm.add_stop_text and set_fsm (the byte automaton is uploaded, expanded over the vocabulary by k_fsm_expand_search and
              checked on the device);
     table    the same automaton expanded on the host (search_expand, plain C++ on one thread), handed to add_table, and set_fsm
              with its host check and its upload of the whole table.
2. The search expansion's launches alone beside the match expansion's (k_fsm_expand) on the SAME tables: the same state count, the
   same vocabulary, the in-library profiler's events.
3. The sampled step (top-k 40) at 1, 64 and 256 sequences: nobody bound, a text stop on every sequence (strings that never occur, so
   that everybody runs to the length), a schema on every sequence.  Wall time of a generate_fsm call over `steps` new ids divided by
   the steps, prompt pass included in all three alike.  --unbound-only measures the first of the three alone, and --root runs against
   another checkout of this repository (the parent commit's build, for "nobody bound costs what it cost").
Each `repeats` times: the best, the median and the spread (largest minus smallest).  Nothing here is a threshold."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

EOS = 2
STEPS = 48
SCHEMA = {"type": "array", "items": {"type": "object", "properties": {"name": {"type": "string"}, "n": {"type": "integer"}}, "required": ["name", "n"]},
          "minItems": 8}


def stats(xs):
    return {"best": round(min(xs), 3), "median": round(statistics.median(xs), 3), "spread": round(max(xs) - min(xs), 3)}


def stop_strings(n):
    """n distinct strings of 8 bytes, lower-case letters behind a byte no piece of the vocabulary's text starts a word with"""
    g = np.random.default_rng(n)
    out = set()
    while len(out) < n:
        out.add(b"\x7f" + bytes(g.integers(0x61, 0x7B, 7).tolist()))
    return sorted(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    own = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap.add_argument("--root", default=own)
    ap.add_argument("--unbound-only", action="store_true")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    from __graft_entry__ import load_package
    pkg = load_package()
    hip = pkg.hipabi.load(0)
    host = pkg.load_host()
    cfg = host.default_config(4, 3)
    cfg.max_ctx, cfg.n_embd, cfg.n_ffn, cfg.n_layers, cfg.n_heads, cfg.n_kv_heads = 64, 256, 512, 2, 4, 2
    V = cfg.n_vocab
    tok = host.tokenizer(os.path.join(root, "tests", "golden", "tokenizer.bin"))
    vocab = tok.vocab_bytes(V)
    ms = lambda t0: 1e3 * (time.perf_counter() - t0)          # noqa: E731
    res = {"what": f"text automata, {V} ids, {len(vocab[0])} vocabulary bytes; ms; {a.repeats} repeats", "checkout": "own" if root == own else "other"}

    if not a.unbound_only:
        m = host.model(cfg)
        m.load_synthetic(4242)
        res["strings"] = {}
        for n in (1, 16, 256):
            strings = stop_strings(n)
            n256, acc = host.stop_text_dfa(strings)
            rows = len(acc) + 1
            out = {"strings": n, "byte_states": len(acc), "pool_states": rows, "pool_mb": round(rows * V * 2 / 1e6, 1)}
            dev = {"build": [], "set_fsm_parts": [], "total": []}
            tab = {"build": [], "host_expand": [], "add_table": [], "set_fsm": [], "total": []}
            for r in range(a.repeats + 1):                    # (the first round of each route warms allocators and code: left out)
                t0 = time.perf_counter()
                f = pkg.hostabi.Fsm(host, V)
                f.set_vocab(vocab)
                f.add_stop_text(strings)
                t1 = ms(t0)
                m.set_fsm(f)
                t2 = ms(t0)
                if r:
                    dev["build"].append(t1), dev["set_fsm_parts"].append(t2 - t1), dev["total"].append(t2)
                f.close()
                t0 = time.perf_counter()
                f = pkg.hostabi.Fsm(host, V)
                f.set_vocab(vocab)
                f.add_stop_text(strings)
                t1 = ms(t0)
                nxt, flags = f.tables()
                t2 = ms(t0)
                g = pkg.hostabi.Fsm(host, V)
                g.add_table(nxt, flags)
                t3 = ms(t0)
                m.set_fsm(g)
                t4 = ms(t0)
                if r:
                    tab["build"].append(t1), tab["host_expand"].append(t2 - t1), tab["add_table"].append(t3 - t2), tab["set_fsm"].append(t4 - t3)
                    tab["total"].append(t4)
                f.close()
                g.close()
                del nxt
            out["device_route_ms"] = {k: stats(v) for k, v in dev.items()}
            out["table_route_ms"] = {k: stats(v) for k, v in tab.items()}
            out["table_over_device"] = round(statistics.median(tab["total"]) / statistics.median(dev["total"]), 2)
            # the two expansions' launches alone, into a pool that exists, on the same tables
            pool = (hip.alloc(rows * V * 2), hip.alloc(rows + 4), rows)
            for name, launch_fn in (("search", lambda: hip.fsm_expand_search(pool, V, 0, vocab, n256, acc)),
                                    ("match", lambda: hip.fsm_expand(pool, V, 0, vocab, n256, acc, -1))):
                launch_fn()
                launch = []
                for _ in range(a.repeats):
                    hip.prof_enable(True)
                    n0, ms0 = hip.prof_read().get("decode_sample", (0, 0.0))
                    launch_fn()
                    n1, ms1 = hip.prof_read()["decode_sample"]
                    hip.prof_enable(False)
                    assert n1 - n0 == 2
                    launch.append(ms1 - ms0)
                out[name + "_launch_ms"] = stats(launch)
                out[name + "_store_gb_s"] = round((rows - (name == "match")) * V * 2 / 1e9 / (statistics.median(launch) / 1e3), 1)
            pool[0].free()
            pool[1].free()
            res["strings"][str(n)] = out
        m.set_fsm(None)
        m.close()

    # the sampled step
    res["step_ms"] = {}
    P, total = 8, 8 + STEPS
    for n_seq in (1, 64, 256):
        d = host.model(cfg) if n_seq == 1 else host.batch(cfg, n_seq)
        d.load_synthetic(4242)
        prompts = [list(host.synthetic_tokens(P, seed=100 + q, n_vocab=V)) for q in range(n_seq)]
        streams = np.arange(n_seq, dtype=np.uint32)

        def run(start):
            t0 = time.perf_counter()
            if n_seq == 1:
                ids, ended = d.generate_fsm(prompts[0], total, start, -1, 40, 0.9, 7, 0)
                ids, ended = [ids], [ended]
            else:
                ids, ended = d.generate_fsm(prompts, total, start, -1, 40, 0.9, 7, streams)
            t = ms(t0)
            return t / STEPS, sum(len(x) - P for x in ids), int(sum(1 for e in ended if e != 0))

        cases = [("unbound", None)]
        if not a.unbound_only:
            cases += [("stop_text", lambda f: f.add_stop_text(stop_strings(16))), ("schema", lambda f: f.add_json_schema(SCHEMA, EOS, 1))]
        out = {}
        for name, add in cases:
            start = -1
            if add:
                f = pkg.hostabi.Fsm(host, V)
                f.set_vocab(vocab)
                start = add(f)
                d.set_fsm(f)
                out[name + "_pool_states"] = f.n_states
                f.close()
            run(start)
            got = [run(start) for _ in range(a.repeats)]
            out[name] = stats([g[0] for g in got])
            out[name + "_new_ids"], out[name + "_ended_early"] = got[-1][1], got[-1][2]
        d.close()
        res["step_ms"][str(n_seq)] = out
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
