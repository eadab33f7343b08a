"""the rows and requests of tests/test_nucleus_gpu.py's operator test, shared with tests/test_nucleus_cpu.py, which checks from the
restatement alone that they are a fair input: at least 90 % of them have their cut clear of every prefix sum by more than
expf's error can move it (nucleus_ref.Cut.near)."""
import numpy as np

VOCABS = [1, 63, 64, 1000, 32003, 65535]
ROWS = 64
TEMPS = [0.7, 1.0, 1.5]
TOP_PS = [0.05, 0.5, 0.9, 0.99, 1.0]
MIN_PS = [0.0, 0.05, 0.5, 1.0]
SEED = 0x5EED_0F_C0FFEE


def top_ks(n_vocab):
    return [1, 40, 1000, n_vocab]


def rows(n_vocab):
    """ROWS rows of N(0, 3^2) logits; every fifth row (1, 6, ...) on a grid of 1/2 (many ties), every seventh (2, 9, ...) with a
    tenth of its entries at -inf -- strides coprime to the four top_k of requests(), so that each kind of row meets each top_k"""
    r = np.random.default_rng(1000 + n_vocab)
    x = (r.standard_normal((ROWS, n_vocab)) * 3.0).astype(np.float32)
    x[1::5] = (np.round(x[1::5] * 2.0) / 2.0).astype(np.float32)
    if n_vocab >= 10:
        for q in range(2, ROWS, 7):
            x[q, r.choice(n_vocab, n_vocab // 10, replace=False)] = -np.inf
    return x


def requests(n_vocab):
    """per row: top_k, temp, top_p, min_p, stream, position -- every (top_k, top_p) pair at least three times, every min_p and temp
    beside every top_p"""
    q = np.arange(ROWS)
    r = np.random.default_rng(2000 + n_vocab)
    ks = np.array(top_ks(n_vocab))[q % 4].astype(np.int32)
    top_p = np.array(TOP_PS)[(q // 4) % 5].astype(np.float32)
    min_p = np.array(MIN_PS)[(q // 20 + q) % 4].astype(np.float32)
    temps = np.array(TEMPS)[(q // 5) % 3].astype(np.float32)
    streams = r.integers(0, 1 << 32, ROWS, dtype=np.uint64).astype(np.uint32)
    pos = r.integers(1, 1 << 20, ROWS).astype(np.int32)
    return ks, temps, top_p, min_p, streams, pos
