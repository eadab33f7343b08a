"""The definitions of include/gten_hip_calib.h in NumPy: the Q4 delta search in f32, one rounding per operation, vectorised over
blocks, with the block sum S written out as its 8-step loop and its tree; the column energy in float64."""
import importlib

import numpy as np

from __graft_entry__ import load_package

load_package()
convert = importlib.import_module("tinyllama_cpp_amd.convert")

F = np.float32


def block_sum(t):
    """S of the header over the last axis (32 f32 terms)"""
    t = t.reshape(t.shape[:-1] + (4, 8))
    p = np.zeros(t.shape[:-1], F)
    for i in range(8):
        p = p + t[..., i]
    return (p[..., 0] + p[..., 1]) + (p[..., 2] + p[..., 3])


def unpack_stream(stream, rows, nb):
    """.gten Q4 block stream -> (f16 deltas [rows][nb], quants f32 [rows][nb][32])"""
    blocks = np.ascontiguousarray(stream).reshape(rows, nb, 18)
    d = np.ascontiguousarray(blocks[:, :, :2]).view(np.float16)[..., 0]
    q = np.concatenate([blocks[:, :, 2:] >> 4, blocks[:, :, 2:] & 15], axis=2).astype(F) - F(7)
    return d, q


def search_q4(w_f32, importance, src, with_choice=False):
    """the block stream gten_hip_quantize_weight_search leaves (before packing); with_choice: also the winning candidate per block"""
    x = np.ascontiguousarray(w_f32, F)
    rows, cols = x.shape
    nb = cols // 32
    with np.errstate(over="ignore"):                             # (an amax / 7 beyond f16 becomes an infinite delta, on purpose)
        out = convert.quantize(x, "q4", src).reshape(rows, nb, 18).copy()
    bd, bq = unpack_stream(out, rows, nb)                        # candidate 0
    x = x.reshape(rows, nb, 32)
    w = np.ones(cols, F) if importance is None else np.asarray(importance, F)
    w = np.broadcast_to(w.reshape(1, nb, 32), x.shape)
    amax = np.abs(x).max(axis=2)
    search = (amax > 0) & np.isfinite(amax) & np.isfinite(bd) & (bd != 0)
    choice = np.zeros((rows, nb), np.int32)
    with np.errstate(all="ignore"):
        def err(d, q):
            e = x - d.astype(F)[..., None] * q
            return block_sum(w * (e * e))
        best = err(bd, bq)
        for c in range(1, 17):
            inv = (F(7.0) + F(0.125) * F(c - 7)) / amax
            q = np.clip(np.rint(x * inv[..., None]), F(-7), F(7))
            a, b = block_sum(w * (x * q)), block_sum(w * (q * q))
            d = (a / b).astype(np.float16)
            e = err(d, q)
            better = search & (b > 0) & np.isfinite(d) & (d != 0) & (e < best)
            best, bd, choice = np.where(better, e, best), np.where(better, d, bd), np.where(better, c, choice)
            bq = np.where(better[..., None], q, bq)
    won = choice > 0
    nib = (bq[won] + F(7)).astype(np.uint8)
    out[won] = np.concatenate([bd[won].reshape(-1, 1).view(np.uint8), (nib[:, :16] << 4) | nib[:, 16:]], axis=1)
    out = out.reshape(rows, nb * 18)
    return (out, choice) if with_choice else out


def col_energy(rows_f32):
    """per column, the float64 sum over rows of the f32 square"""
    x = np.asarray(rows_f32, F)
    return (x * x).astype(np.float64).sum(axis=0)
