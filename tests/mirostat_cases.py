"""the rows and requests of tests/test_mirostat_gpu.py's operator test, shared with tests/test_mirostat_cpu.py, which checks from the
restatement alone that they are a fair input: at most 10 % of the rows have a candidate that expf's error can move across the threshold
(miro_ref.Step.near), and at least 10 % are cut properly (1 < n_keep < n_cand).

The rows, top_k, temperature, stream and position are tests/nucleus_cases.py's; tau and eta are one pair; mu cycles through eight values
with a stride of four rows, so that every mu meets every top_k."""
import numpy as np

import nucleus_cases as ncases

VOCABS = ncases.VOCABS
ROWS = ncases.ROWS
SEED = ncases.SEED
TAU, ETA = 5.0, 0.1
TAU_Q, ETA_Q = 5 << 16, 6554
MUS = [0, 1, 3, 6, 10, 16, 40, -1]                  # bits


def rows(n_vocab):
    return ncases.rows(n_vocab)


def requests(n_vocab):
    """per row: top_k, temp, stream, position, mu (Q16)"""
    ks, temps, _, _, streams, pos = ncases.requests(n_vocab)
    q = np.arange(ROWS)
    mus = (np.array(MUS, np.int64)[(q // 4) % 8] << 16).astype(np.int32)
    return ks, temps, streams, pos, mus
