"""Stop strings given as text, restated in Python for the tests (include/gten_host_stoptext.h): the automaton by
brute-force suffix tests, the search expansion as a walk per (state, id), and where to cut.  It runs none of the project's code."""
import numpy as np

DEAD = 0xFFFF


def dfa(strings):
    """(next256 u16 [S][256], accept u8 [S]).  A state is a prefix of some string; numbered breadth first from the empty prefix with
    bytes ascending.  next[p][b] = the longest suffix of p + b that is a prefix; accept[p] = some string is a suffix of p."""
    strings = [bytes(s) for s in strings]
    prefixes = {s[:k] for s in strings for k in range(len(s) + 1)}
    order, head = [b""], 0
    while head < len(order):
        p = order[head]
        head += 1
        order += [p + bytes([b]) for b in range(256) if p + bytes([b]) in prefixes]
    number = {p: k for k, p in enumerate(order)}
    assert len(number) == len(prefixes)
    nxt, acc = np.zeros((len(order), 256), np.uint16), np.zeros(len(order), np.uint8)
    for p, k in number.items():
        acc[k] = any(p.endswith(s) for s in strings)
        for b in range(256):
            q = p + bytes([b])
            while q not in prefixes:
                q = q[1:]
            nxt[k][b] = number[q]
    return nxt, acc


def expand(n256, acc, pieces, base):
    """(rows u16 [Sb + 1][V], flags u8 [Sb + 1]) by the search rule: an empty piece stays, a piece that passes an accepting state enters
    the HIT state base + Sb, an automaton entry >= Sb kills"""
    Sb, V = len(acc), len(pieces)
    rows = np.full((Sb + 1, V), DEAD, np.uint16)
    for s in range(Sb):
        for i, p in enumerate(pieces):
            cur, hit = s, False
            for c in p:
                cur = int(n256[cur][c])
                if cur >= Sb:
                    cur = -1
                    break
                hit = hit or bool(acc[cur])
            rows[s][i] = DEAD if cur < 0 else base + (Sb if hit else cur)
    return rows, np.array([0] * Sb + [1], np.uint8)


def find(strings, text):
    """(index, begin, end): the match that ends first; among those the longest; among equal ones the lowest index; (-1, n, n) for none"""
    strings, text = [bytes(s) for s in strings], bytes(text)
    for end in range(1, len(text) + 1):
        here = [(-len(s), k) for k, s in enumerate(strings) if len(s) <= end and text[end - len(s):end] == s]
        if here:
            neg, k = min(here)
            return k, end + neg, end
    return -1, len(text), len(text)


def clamp_pieces(vb, vo, n_bytes):
    """the pieces the device reads from offsets that may lie outside [0, n_bytes] or run backwards: within a tile of 256 ids every offset
    is clamped into the tile's own byte range, and a piece that would end before it begins is empty (csrc/gten_fsm_search.h)"""
    V, raw, out = len(vo) - 1, bytes(np.asarray(vb, np.uint8)), []
    cl = lambda v, lo, hi: lo if v < lo else (hi if v > hi else v)      # noqa: E731
    for t0 in range(0, V, 256):
        t1 = min(t0 + 256, V)
        tile_lo = cl(int(vo[t0]), 0, n_bytes)
        tile_hi = cl(int(vo[t1]), tile_lo, n_bytes)
        for t in range(t0, t1):
            lo = cl(int(vo[t]), tile_lo, tile_hi)
            hi = cl(int(vo[t + 1]), lo, tile_hi)
            out.append(raw[lo:hi])
    return out
