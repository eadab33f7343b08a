"""The dequantisation of GPTQ and AWQ (GEMM) 4-bit tensors that include/gten_hip_w4.h defines, restated in NumPy, and random
sources for it.  What tests/test_w4_gpu.py and tests/test_w4_cpu.py compare against.

Our weight is [N out][K in].  G groups = K / group_size (1 for -1).  P = [0, 4, 1, 5, 2, 6, 3, 7].
    gptq   qweight int32 [K/8][N]   q(k, n) = (qweight[k >> 3][n] >> 4 (k & 7)) & 15
           qzeros  int32 [G][N/8]   z(g, n) = ((qzeros[g][n >> 3] >> 4 (n & 7)) & 15) + zero_offset       (no wrap: z may be 16)
    awq    qweight int32 [K][N/8]   q(k, n) = (qweight[k][n >> 3] >> 4 P[n & 7]) & 15
           qzeros  int32 [G][N/8]   z(g, n) = (qzeros[g][n >> 3] >> 4 P[n & 7]) & 15
    scales f16 [G][N];  g(k) = g_idx[k] if there is one, else k / group_size
    D(n, k) = to_f16((float)(q - z) * widen(scales[g][n]))"""
import numpy as np

P = np.array([0, 4, 1, 5, 2, 6, 3, 7])


def _nibbles(words, order):
    """int32 [R][C] -> [R][8 C]: nibble order[j] of word c is element 8 c + j"""
    w = np.ascontiguousarray(words).view(np.uint32)
    return ((w[:, :, None] >> (4 * order)[None, None, :].astype(np.uint32)) & 15).astype(np.int32).reshape(w.shape[0], -1)


def dequant(layout, qweight, qzeros, scales, g_idx, zero_offset, group_size):
    """-> f32 [N][K] holding the f16 values D(n, k)"""
    if layout == "gptq":
        kw, n = qweight.shape
        q = _nibbles(np.ascontiguousarray(qweight.T), np.arange(8)).reshape(n, kw * 8).T          # [K][N]
        z = _nibbles(qzeros, np.arange(8)) + zero_offset                                           # [G][N]
    else:
        q, z = _nibbles(qweight, P), _nibbles(qzeros, P)
    k = q.shape[0]
    g = np.asarray(g_idx) if g_idx is not None else np.arange(k) // (k if group_size == -1 else group_size)
    with np.errstate(over="ignore", invalid="ignore"):
        d = (q - z[g]).astype(np.float32) * scales.astype(np.float32)[g]                           # [K][N], exact in f32
        return np.ascontiguousarray(d.T.astype(np.float16).astype(np.float32))


def random_source(layout, n, k, group_size, rng, act_order=False, scale_max=0.05):
    """(qweight, qzeros, scales, g_idx or None): every word uniform (so every nibble, the zeros' too, takes all 16 values), scales
    finite f16 in (-scale_max, scale_max); act_order: g_idx a random permutation of k / group_size (blocks straddle groups)"""
    groups = 1 if group_size == -1 else k // group_size
    words = lambda *shape: rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32).view(np.int32)      # noqa: E731
    qweight = words(k // 8, n) if layout == "gptq" else words(k, n // 8)
    scales = rng.uniform(-scale_max, scale_max, (groups, n)).astype(np.float16)
    g_idx = rng.permutation(np.arange(k) // (k // groups)).astype(np.int32) if act_order else None
    return qweight, words(groups, n // 8), scales, g_idx
