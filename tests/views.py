"""Row views for the operator tests: rows laid into a parent buffer at a base offset and a pitch, canaries everywhere else.

An operator of include/gten_hip.h sees a matrix as a base pointer and a pitch; of a row only its first `row_bytes` belong to it.
The parent buffer built here is what the device holds around such a view:

    [ HEAD bytes | offset bytes | row 0 | padding | row 1 | padding | ... | row n-1 | padding | GUARD bytes ]
                                ^ the view's base = HEAD + offset (HEAD is a multiple of 256, as the allocation's start is)

Everything but the rows is canary bytes -- a pattern that changes from byte to byte, so that a stray store of any constant is
seen.  `outside_untouched` is the assertion the GPU tests make on every output parent; tests/test_views_cpu.py shows that it
fails on one flipped byte of every region it is meant to guard.
"""
import numpy as np

HEAD = 256         # the view's base offset is counted from a 256-aligned address inside the parent
GUARD = 64         # bytes watched before the first row and after the last row's padding

# (base offset, pitch - row_bytes) in bytes
CONTROL = (0, 0)
CLASSES = [CONTROL,             # dense rows at an aligned base
           (16, 16),            # non-dense, every fast kernel still applies
           (8, 8), (4, 4),      # fails 16, passes 4
           (2, 2), (2, 14),     # 2-byte aligned only
           (34, 34)]            # ... as the Q8 column range from block 1 of rows one block wider


def canaries(nbytes, fill):
    """`nbytes` canary bytes: `fill` at byte 0, then a stride-131 walk over all 256 values"""
    return ((np.arange(nbytes, dtype=np.int64) * 131 + int(fill)) & 0xFF).astype(np.uint8)


def parent_size(offset, pitch, n):
    return HEAD + offset + n * pitch + GUARD


def base(offset):
    """where the view starts inside its parent"""
    return HEAD + offset


def _row_index(offset, pitch, n, row_bytes, first=0):
    """indices into the parent of the bytes of rows [first, n)"""
    assert 0 <= offset and row_bytes <= pitch and 0 <= first <= n
    r = np.arange(first, n, dtype=np.int64)[:, None] * pitch + np.arange(row_bytes, dtype=np.int64)[None, :]
    return (base(offset) + r).reshape(-1)


def embed(rows_u8, offset, pitch, fill):
    """the parent bytes: `rows_u8` (uint8 [n][row_bytes]) at HEAD + offset + r * pitch, canaries everywhere else"""
    rows = np.ascontiguousarray(rows_u8).view(np.uint8)
    assert rows.ndim == 2
    n, row_bytes = rows.shape
    parent = canaries(parent_size(offset, pitch, n), fill)
    parent[_row_index(offset, pitch, n, row_bytes)] = rows.reshape(-1)
    return parent


def extract(parent, offset, pitch, n, row_bytes):
    """the rows of the view, uint8 [n][row_bytes] (a copy)"""
    parent = np.ascontiguousarray(parent).view(np.uint8).reshape(-1)
    assert parent.size == parent_size(offset, pitch, n), (parent.size, parent_size(offset, pitch, n))
    return parent[_row_index(offset, pitch, n, row_bytes)].reshape(n, row_bytes).copy()


def outside_untouched(parent_before, parent_after, offset, pitch, n, row_bytes, start_pos=0, what=""):
    """every byte of the parent outside [base + r * pitch, + row_bytes) of the WRITTEN rows r in [start_pos, n) is unchanged:
    both guards, the bytes before the base, the padding of every row (the last one's included) and the rows below start_pos"""
    before = np.ascontiguousarray(parent_before).view(np.uint8).reshape(-1)
    after = np.ascontiguousarray(parent_after).view(np.uint8).reshape(-1)
    assert before.size == after.size == parent_size(offset, pitch, n), (what, before.size, after.size)
    free = np.zeros(before.size, bool)
    free[_row_index(offset, pitch, n, row_bytes, start_pos)] = True
    bad = np.flatnonzero(~free & (before != after))
    if bad.size:
        i = int(bad[0])
        rel = i - base(offset)
        where = ("before the view" if rel < 0 else "behind the last row's padding" if rel >= n * pitch else
                 f"row {rel // pitch}, byte {rel % pitch} of pitch {pitch} (row_bytes {row_bytes}, start_pos {start_pos})")
        raise AssertionError(f"{what}: {bad.size} bytes outside the written rows changed; the first at parent byte {i}: {where}, "
                             f"{before[i]:#04x} -> {after[i]:#04x}")
