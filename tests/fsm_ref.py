"""brute-force restatement of the token automata's contract (include/gten_hip_fsm.h) in plain Python / numpy: the walk of
a pool's tables, the stop scan, the masked row, and small builders of the pools the tests use.  Nothing here is shared with the code
under test."""
import numpy as np

DEAD = 0xFFFF
FINAL = 1
MAX_STATES = 65535
MAX_BYTES = 1 << 30
OK, BAD_STATES, TOO_LARGE, BAD_ENTRY, STUCK = 0, 1, 2, 3, 4


def walk(nxt, flags, start, ids):
    """the states entered by `ids` from `start`: states[i] is the state after ids[i].  The walk stops being advanced at a final state
    (the sequence has ended there: the state is carried on) and at a banned id (DEAD from then on)."""
    s, out = int(start), []
    for t in ids:
        if s != DEAD and not (flags[s] & FINAL):
            s = int(nxt[s][t])
        out.append(s)
    return out


def first_final(nxt, flags, start, ids):
    """the index of the first id that enters a final state, or None"""
    for i, s in enumerate(walk(nxt, flags, start, ids)):
        if s != DEAD and flags[s] & FINAL:
            return i
    return None


def stop_scan(ids, stops):
    """the first position at which any stop sequence ends, by direct scan: the smallest i such that ids[i - len(s) + 1 .. i] == s for
    some s; None when there is none"""
    ids = list(ids)
    for i in range(len(ids)):
        for s in stops:
            s = list(s)
            if len(s) <= i + 1 and ids[i + 1 - len(s): i + 1] == s:
                return i
    return None


def trie_edges(choices):
    """{prefix tuple: set of ids that may follow it} of a choice list, and the set of complete choices"""
    edges = {}
    for c in choices:
        for i in range(len(c)):
            edges.setdefault(tuple(c[:i]), set()).add(int(c[i]))
    return edges, {tuple(c) for c in choices}


def mask_row(x, nxt, flags, state):
    """the row the draw is made from: x where the state allows the id, -inf where it does not; a final state, or -1, masks nothing.
    Allowed logits keep their bits."""
    x = np.asarray(x, np.float32)
    if state < 0 or flags[state] & FINAL:
        return x.copy()
    y = x.copy()
    y[np.asarray(nxt[state]) == DEAD] = -np.inf
    return y


def bias_of(nxt, flags, state, n_vocab):
    """the 0 / -inf bias row that restates the mask of `state` for the existing operators"""
    b = np.zeros(n_vocab, np.float32)
    if state >= 0 and not (flags[state] & FINAL):
        b[np.asarray(nxt[state]) == DEAD] = -np.inf
    return b


def check(nxt, flags, n_states, n_vocab):
    """the upload validation that needs no device, restated: a code as in include/gten_hip_fsm.h"""
    if nxt is None or flags is None or n_states < 1 or n_states > MAX_STATES or n_vocab < 1:
        return BAD_STATES
    if n_states * n_vocab * 2 > MAX_BYTES:
        return TOO_LARGE
    for s in range(n_states):
        row = np.asarray(nxt[s])
        live = row[row != DEAD]
        if (live >= n_states).any():
            return BAD_ENTRY
        if len(live) == 0 and not (flags[s] & FINAL):
            return STUCK
    return OK


def random_pool(g, n_states, n_vocab, density=0.25, n_final=1, pin=()):
    """a pool of n_states states whose live states allow about `density` of the ids (at least one), leading to random states; the
    last n_final states are final.  pin: (state, id, allowed) triples forced afterwards."""
    nxt = g.integers(0, n_states, (n_states, n_vocab)).astype(np.uint16)
    nxt[g.random((n_states, n_vocab)) >= density] = DEAD
    flags = np.zeros(n_states, np.uint8)
    flags[n_states - n_final:] = FINAL
    for s, i, allowed in pin:
        nxt[s, i] = g.integers(0, n_states) if allowed else DEAD
    for s in range(n_states):
        if (nxt[s] == DEAD).all():
            nxt[s, g.integers(0, n_vocab)] = g.integers(0, n_states)
    return nxt, flags
