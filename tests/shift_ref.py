"""The context shift's reference (include/gten_hip_shift.h), on storage bytes in numpy.

unrot(row, d) is defined through the operator that exists already: swap the two halves of every head of the stored row, apply
the oracle's rotary_emb at row index d, swap the halves back.  V is row copies.  Nothing here knows the direction of a rotation or
a quantiser of its own: the swaps are byte moves and the arithmetic is oracle/orc.py's."""
import numpy as np

from oracle import orc

F16, Q8 = orc.F16, orc.Q8


def swap_halves(rows, dtype, kv_dim, d_head):
    """uint8 [n][row_bytes] with the two halves of every head exchanged (a byte move; its own inverse)"""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    n, half = rows.shape[0], d_head // 2
    out = rows.copy()
    if dtype == F16:
        v = rows.view(np.uint16).reshape(n, kv_dim // d_head, 2, half)
        out.view(np.uint16).reshape(n, kv_dim // d_head, 2, half)[:] = v[:, :, ::-1, :]
    elif d_head == 64:      # the head's two 34-byte blocks, whole, deltas included
        v = rows.reshape(n, kv_dim // 64, 2, 34)
        out.reshape(n, kv_dim // 64, 2, 34)[:] = v[:, :, ::-1, :]
    elif d_head == 32:      # the two 16-quant halves inside the block, which share one delta
        v = rows.reshape(n, kv_dim // 32, 34)
        o = out.reshape(n, kv_dim // 32, 34)
        o[:, :, 2:18] = v[:, :, 18:34]
        o[:, :, 18:34] = v[:, :, 2:18]
    else:
        raise ValueError(d_head)
    return out


def unrot_rows(lib, rows, dtype, kv_dim, d_head, d):
    """unrot of every row of uint8 [n][row_bytes] by d positions"""
    sw = swap_halves(rows, dtype, kv_dim, d_head)
    buf = np.zeros((d + 1, sw.shape[1]), np.uint8)
    for r in range(sw.shape[0]):
        buf[d] = sw[r]
        lib.rotary_emb(buf, dtype, d + 1, kv_dim, d_head, start_pos=d)
        sw[r] = buf[d]
    return swap_halves(sw, dtype, kv_dim, d_head)


def shift_ref(lib, k, v, dtype, kv_dim, d_head, n, keep, drop):
    """(k, v) after shift(keep, drop) of caches uint8 [rows][pitch] whose rows [0, n) are valid: copies, the inputs are left alone.
    Only bytes [0, row_bytes) of rows [keep, keep + m) differ from the inputs."""
    assert 0 <= keep and 1 <= drop and keep + drop <= n
    rb = orc.row_bytes(dtype, kv_dim)
    m = n - keep - drop
    k2, v2 = k.copy(), v.copy()
    if m > 0:
        k2[keep:keep + m, :rb] = unrot_rows(lib, k[keep + drop:n, :rb], dtype, kv_dim, d_head, drop)
        v2[keep:keep + m, :rb] = v[keep + drop:n, :rb]
    return k2, v2


def phi(p, keep, drop):
    """where position p of the old sequence lies after shift(keep, drop)"""
    return p if p < keep else keep if p < keep + drop else p - drop


def shift_ids(ids, keep, drop):
    return list(ids[:keep]) + list(ids[keep + drop:])
