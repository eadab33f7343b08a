"""A float64 restatement of the log-prob record (include/gten_hip_logprobs.h) in plain numpy: lse in float64, the
order of the alternatives on the f32 values with -0 == +0 and ties to the lower index."""
import numpy as np

TOP = 20            # GTEN_HIP_LOGPROBS_TOP


def key(x):
    """the order-preserving integer image of f32 values (larger float -> larger key; -0 and +0 share one key)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.int64)
    u = np.where(u == 0x80000000, 0, u)
    return np.where(u & 0x80000000, 0xFFFFFFFF - u, u | 0x80000000)


def lse(x):
    x = np.asarray(x, np.float32).astype(np.float64)
    m = x.max()
    return m + np.log(np.exp(x - m).sum())


def order(x):
    """every index, by (value descending, index ascending)"""
    k = key(x)
    return np.lexsort((np.arange(len(k)), -k))


def record(x, n_top, chosen=-1):
    """(logprob, top_id int64[n_top], top_logprob float64[n_top]) of the row x with the chosen id (-1: none -> logprob 0);
    entries from min(n_top, len(x)) on are -1 / 0"""
    x = np.asarray(x, np.float32)
    L = lse(x)
    m = min(n_top, len(x))
    ids = np.full(n_top, -1, np.int64)
    lps = np.zeros(n_top, np.float64)
    ids[:m] = order(x)[:m]
    lps[:m] = x[ids[:m]].astype(np.float64) - L
    lp = float(x[chosen]) - L if 0 <= chosen < len(x) else 0.0
    return lp, ids, lps


def rank(x, chosen):
    """how many ids precede `chosen` under (value descending, index ascending)"""
    return int(np.flatnonzero(order(x) == chosen)[0])
