"""A numpy restatement of beam search as include/gten_hip_beam.h and host/beam_plan.h define it: the round in f32
with every operation rounded once, the length weights, the walk back through the trellis, the final ranking, and a whole search
over a caller-supplied function lists(prefix ids) -> (top_id[2B], top_lp[2B])."""
import math

import numpy as np

BEAM_MAX = 8
F = np.float32
# gten_hip_beam_state: 176 bytes
STATE = np.dtype([("cum", np.float32, 8), ("fin_final", np.float32, 8), ("fin_cum", np.float32, 8), ("fin_t", np.int32, 8),
                  ("fin_beam", np.int32, 8), ("n_fin", np.int32), ("done", np.int32), ("t", np.int32), ("stepped", np.int32)])
assert STATE.itemsize == 176


def new_state():
    return np.zeros(1, STATE)[0]


def weights(max_new, length_penalty):
    w = np.zeros(max_new + 1, np.float32)
    for t in range(1, max_new + 1):
        w[t] = F(1.0 / math.pow(float(t), float(F(length_penalty))))
    return w


def round_(st, top_id, top_lp, n_beams, eos, w, max_new, trace=None):
    """one round of one group, in place on the STATE record `st`; top_id / top_lp: [>= n_beams][>= 2 n_beams].  Returns
    (parent int32[8], ids int32[8], next ids int32[n_beams]) -- entries from n_beams on are 0 --, or None where the group is left alone.
    trace (a list): what became of every eos candidate walked: 'finish' | 'drop' | 'replace' | 'keep'."""
    trace = [] if trace is None else trace
    B, L = n_beams, 2 * n_beams
    if st["done"]:
        return None
    t = int(st["t"]) + 1
    if t > max_new:
        st["stepped"] = 0
        return None
    n_src = 1 if t == 1 else B
    cand = []
    for b in range(n_src):
        for r in range(L):
            cand.append((F(st["cum"][b]) + F(top_lp[b][r]), b, r, int(top_id[b][r])))
    cand.sort(key=lambda c: (-float(c[0]), c[1], c[2]))
    cand = cand[:L]
    parent, ids = np.zeros(8, np.int32), np.zeros(8, np.int32)
    cum = st["cum"].copy()
    n_next, n_fin = 0, int(st["n_fin"])
    for k, (score, b, r, tok) in enumerate(cand):
        if n_next == B:
            break
        if eos >= 0 and tok == eos:
            if k >= B:
                trace.append("drop")
                continue
            fin = F(score) * F(w[t])
            slot = -1
            if n_fin < B:
                slot, n_fin = n_fin, n_fin + 1
                trace.append("finish")
            else:
                lo = 0
                for j in range(1, B):
                    if st["fin_final"][j] <= st["fin_final"][lo]:
                        lo = j
                if fin > st["fin_final"][lo]:
                    slot = lo
                trace.append("replace" if slot >= 0 else "keep")
            if slot >= 0:
                st["fin_final"][slot], st["fin_cum"][slot], st["fin_t"][slot], st["fin_beam"][slot] = fin, score, t, b
        else:
            parent[n_next], ids[n_next], cum[n_next] = b, tok, score
            n_next += 1
    assert n_next == B, "a source lists eos at most once"
    st["cum"] = cum
    st["n_fin"], st["done"], st["t"], st["stepped"] = n_fin, 1 if n_fin >= B else 0, t, 1
    return parent, ids, ids[:B].copy()


def backtrack(parent, ids, t, b):
    """the ids of beam b after round t; round r's row at index r - 1"""
    out = []
    for r in range(t, 0, -1):
        out.append(int(ids[r - 1][b]))
        b = int(parent[r - 1][b])
    return out[::-1]


def finalize(st, parent, ids, n_beams, w):
    """[(ids, final f32, cum f32, 'eos' | 'length')], best first"""
    items = []
    for s in range(min(int(st["n_fin"]), n_beams)):
        items.append((F(st["fin_final"][s]), 0, s))
    if not st["done"] and st["t"] >= 1:
        for b in range(n_beams):
            items.append((F(st["cum"][b]) * F(w[int(st["t"])]), 1, b))
    items.sort(key=lambda x: (-float(x[0]), x[1], x[2]))
    out = []
    for fin, live, at in items[:n_beams]:
        if live:
            out.append((backtrack(parent, ids, int(st["t"]), at), F(fin), F(st["cum"][at]), "length"))
        else:
            out.append((backtrack(parent, ids, int(st["fin_t"][at]) - 1, int(st["fin_beam"][at])), F(fin), F(st["fin_cum"][at]), "eos"))
    return out


def search(lists, n_beams, max_new, eos, w):
    """a whole search of one group: lists(tuple of new ids so far) -> (top_id[2B], top_lp[2B]) of the row behind that prefix.
    Returns (state, parent rows, id rows, hypotheses)"""
    B = n_beams
    st = new_state()
    parent, ids = [], []
    for _ in range(max_new):
        t = int(st["t"])
        n_src = 1 if t == 0 else B
        ti, tl = np.zeros((B, 2 * B), np.int32), np.zeros((B, 2 * B), np.float32)
        for b in range(n_src):
            ti[b], tl[b] = lists(tuple(backtrack(parent, ids, t, b)))
        got = round_(st, ti, tl, B, eos, w, max_new)
        if got is None:
            break
        parent.append(got[0])
        ids.append(got[1])
        if st["done"]:
            break
    return st, parent, ids, finalize(st, parent, ids, B, w)
