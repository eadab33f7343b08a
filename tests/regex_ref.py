"""The meaning of a regular expression's byte automaton, restated in Python for the tests (include/gten_host_regex.h, DESIGN.md
3.18): acceptance of a byte string, and the expansion over a vocabulary as a walk per (state, id).  It runs none of the project's code."""
import numpy as np

DEAD = 0xFFFF
NONE = 0xFFFF


def accepts(n256, acc, data):
    s = 0
    for c in data:
        s = int(n256[s][c])
        if s == NONE:
            return False
    return bool(acc[s])


def pieces_of(vocab):
    vb, vo = vocab
    raw = bytes(np.asarray(vb, np.uint8))
    return [raw[vo[i]:vo[i + 1]] for i in range(len(vo) - 1)]


def expand(n256, acc, pieces, eos, base):
    """(rows u16 [Sb (+ 1)][V], flags u8 [Sb (+ 1)]): the walk of every piece from every state, all ids at once per byte position"""
    Sb, V = len(acc), len(pieces)
    lens = np.array([len(p) for p in pieces])
    text = np.zeros((V, max(int(lens.max()), 1)), np.int64)
    for i, p in enumerate(pieces):
        text[i, :len(p)] = list(p)
    edges = (np.asarray(n256) != NONE).any(axis=1)
    rows = np.full((Sb + (eos >= 0), V), DEAD, np.uint16)
    for s in range(Sb):
        cur = np.where(lens > 0, s, -1)
        for j in range(text.shape[1]):
            on = (cur >= 0) & (lens > j)
            nxt = np.asarray(n256, np.int64)[np.maximum(cur, 0), text[:, j]]
            cur = np.where(on, np.where(nxt == NONE, -1, nxt), cur)
        rows[s] = np.where(cur < 0, DEAD, base + cur)
        if eos >= 0:
            rows[s][eos] = base + Sb if (acc[s] and edges[s]) else DEAD
    flags = np.array([1 if (acc[s] and not edges[s]) else 0 for s in range(Sb)] + [1] * (eos >= 0), np.uint8)
    return rows, flags


def synthetic_vocab(n_vocab, seed, alphabet=b"ab01 .\n", long_piece=0, extra=()):
    """n_vocab pieces over `alphabet`: id 0 empty, every single byte of the alphabet, then random pieces of 1 to 5 bytes with an empty
    one now and then; `extra` pieces are placed at the end, and with long_piece > 0 one piece of that many bytes ('a' repeated) sits
    in the middle"""
    g = np.random.default_rng(seed)
    out = [b""] + [bytes([c]) for c in alphabet]
    while len(out) < n_vocab:
        n = int(g.integers(0, 6))
        out.append(bytes(g.choice(list(alphabet), n).tolist()) if n and g.integers(0, 17) else b"")
    out = out[:n_vocab]
    if long_piece and n_vocab > 2:
        out[n_vocab // 2] = b"a" * long_piece
    for k, e in enumerate(extra):
        if n_vocab - 1 - k >= 0:
            out[n_vocab - 1 - k] = e
    return out
