"""The definition of include/gten_hip_embed.h restated in numpy with explicit float32 / float64 operations in the stated order, and the
plan of host/embed_plan.h restated in Python.  Nothing here touches a device."""
import numpy as np

F16, Q8 = 1, 3                          # dtype codes of include/gten_hip.h
CHUNK = 64
GROUP_TEXTS, GROUP_ROWS, GROUP_MIN, GROUP_MAX = 32, 4096, 16, 2048


def row_bytes(dtype, n_embd):
    return n_embd * 2 if dtype == F16 else n_embd // 32 * 34


def rows_to_f32(rows, dtype):
    """x[r][c]: the storage value as f32.  rows: uint8 [n][row bytes]"""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    if dtype == F16:
        return rows.view(np.float16).astype(np.float32)
    blk = rows.reshape(rows.shape[0], -1, 34)
    d = np.ascontiguousarray(blk[:, :, :2]).view(np.float16).astype(np.float32)          # f16_to_f32(delta)
    q = np.ascontiguousarray(blk[:, :, 2:]).view(np.int8).astype(np.float32)             # (float)q
    return np.multiply(q, d, dtype=np.float32).reshape(rows.shape[0], -1)                # one f32 multiply


def pack_q8(q, delta):
    """Q8 rows from int8 q [n][n_embd] and float16 delta [n][n_embd / 32]: uint8 [n][n_embd / 32 * 34]"""
    n, e = q.shape
    out = np.zeros((n, e // 32, 34), np.uint8)
    out[:, :, :2] = np.ascontiguousarray(delta, dtype=np.float16).view(np.uint8).reshape(n, e // 32, 2)
    out[:, :, 2:] = np.ascontiguousarray(q, dtype=np.int8).view(np.uint8).reshape(n, e // 32, 32)
    return out.reshape(n, -1)


def mean_f32(x):
    """m of mean pooling for one segment, x: f32 [n][n_embd]"""
    x = np.asarray(x, dtype=np.float32)
    n = x.shape[0]
    s = None
    for j in range(0, n, CHUNK):
        p = x[j].copy()                                          # a sum starts from its first term
        for r in range(j + 1, min(j + CHUNK, n)):
            p = np.add(p, x[r], dtype=np.float32)
        s = p if s is None else np.add(s, p, dtype=np.float32)
    return np.divide(s, np.float32(n), dtype=np.float32)


def normalize(m):
    m = np.asarray(m, dtype=np.float32)
    sq = np.multiply(m.astype(np.float64), m.astype(np.float64), dtype=np.float64)       # every product is exact
    # t[k] = sq[k] + sq[k + 64] + ... ascending, all 64 k at once.  Columns past the end count as +0: every product is >= +0, and
    # adding +0 to such a value returns it unchanged, so the padded sum is the sum over the columns that exist
    sq = np.concatenate([sq, np.zeros(-len(sq) % 64, np.float64)]).reshape(-1, 64)
    t = sq[0].copy()
    for i in range(1, sq.shape[0]):
        t = np.add(t, sq[i], dtype=np.float64)
    ss = t[0]
    for k in range(1, 64):
        ss = np.add(ss, t[k], dtype=np.float64)
    if ss == 0.0:
        return np.zeros(len(m), np.float32)
    return np.divide(m.astype(np.float64), np.sqrt(ss), dtype=np.float64).astype(np.float32)


def pool(x, pooling="mean", norm=True):
    """the vector of one segment, x: f32 [n][n_embd]"""
    m = mean_f32(x) if pooling == "mean" else np.asarray(x, dtype=np.float32)[-1].copy()
    return normalize(m) if norm else m


def pool_rows(rows, dtype, starts, pooling="mean", norm=True):
    """gten_hip_pool_rows on storage rows (uint8 [rows][row bytes], minimal pitch): f32 [len(starts) - 1][n_embd]"""
    x = rows_to_f32(rows, dtype)
    return np.stack([pool(x[starts[k]:starts[k + 1]], pooling, norm) for k in range(len(starts) - 1)])


def ulps(a, b):
    """distance in f32 units in the last place between two f32 arrays of finite values (+0 and -0 are 0 apart)"""
    def key(v):
        i = np.ascontiguousarray(v, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def plan(lengths, seg_ok=True):
    """host/embed_plan.h: (group of every text, [1 where the group is a text that goes alone]); None: no texts or a text without ids"""
    if len(lengths) < 1 or any(n < 1 for n in lengths):
        return None
    group_of, alone = [], []
    open_g, texts, rows = -1, 0, 0
    for n in lengths:
        if not (seg_ok and GROUP_MIN <= n <= GROUP_MAX):
            group_of.append(len(alone))
            alone.append(1)
            continue
        if open_g < 0 or texts == GROUP_TEXTS or rows + n > GROUP_ROWS:
            open_g, texts, rows = len(alone), 0, 0
            alone.append(0)
        group_of.append(open_g)
        texts += 1
        rows += n
    return group_of, alone
