"""Plain Python restatement of n samples per prompt (include/gten_host_samples.h): the expanded queue, the order of its outputs
and the best-of-n ranking, plus the seeded ranking cases tests/test_samples_cpu.py checks the library against."""
import random

import numpy as np


def first_items(n_samples):
    """first[j]: the expanded queue's item that is sample 0 of prompt j (one more entry: the number of items)"""
    first = [0]
    for n in n_samples:
        first.append(first[-1] + int(n))
    return first


def expand(values, n_samples):
    """a per-prompt list written out per item: prompt j's value n_samples[j] times in a row"""
    out = []
    for v, n in zip(values, n_samples):
        out += [v] * int(n)
    return out


def regroup(items, n_samples):
    """a per-item list cut into per-prompt lists: the inverse of expand's layout"""
    first = first_items(n_samples)
    return [list(items[first[j]: first[j + 1]]) for j in range(len(n_samples))]


def rank(logprob_sum, n_new):
    """the samples' indices, best first: descending mean log-prob per new id (sum / n_new as Python floats -- doubles), ties to the
    lower sample, samples without new ids last (by index)"""
    with_ids = [i for i in range(len(n_new)) if n_new[i] > 0]
    without = [i for i in range(len(n_new)) if n_new[i] == 0]
    mean = {i: float(logprob_sum[i]) / float(n_new[i]) for i in with_ids}
    return sorted(with_ids, key=lambda i: (-mean[i], i)) + without


def record_sums(records, n_prompt, n_new):
    """per sample the sum of its f32 records at positions [n_prompt, n_prompt + n_new), formed in double, added in position order"""
    out = []
    for row, n in zip(records, n_new):
        s = 0.0
        for t in range(int(n)):
            s += float(np.float32(row[n_prompt + t]))
        out.append(s)
    return out


def rank_cases(count=200, seed=20241020):
    """(records f32 [n][width], n_prompt, n_new) triples: 1 .. 12 samples, ties made on purpose (equal rows, equal means from other
    lengths), samples without new ids, a lone sample"""
    rng = random.Random(seed)
    out = []
    while len(out) < count:
        kind = len(out) % 5
        n = 1 if kind == 4 else rng.randrange(2, 13)
        n_prompt = rng.randrange(1, 20)
        width = n_prompt + 12
        rec = np.zeros((n, width), np.float32)
        n_new = [rng.randrange(1, 13) for _ in range(n)]
        for i in range(n):
            for t in range(n_new[i]):
                rec[i, n_prompt + t] = -rng.random() * 6.0
        if kind == 1 and n >= 2:                                   # equal rows: equal means, the lower sample first
            a, b = rng.sample(range(n), 2)
            rec[b] = rec[a]
            n_new[b] = n_new[a]
        if kind == 2 and n >= 2:                                   # equal means from other lengths: -0.5 per id, exact in f32
            a, b = rng.sample(range(n), 2)
            for i, k in ((a, 4), (b, 8)):
                rec[i] = 0
                rec[i, n_prompt: n_prompt + k] = -0.5
                n_new[i] = k
        if kind == 3:                                              # samples without new ids come last
            for i in rng.sample(range(n), max(1, n // 3)):
                n_new[i] = 0
                rec[i] = 0
        out.append((rec, n_prompt, n_new))
    return out
