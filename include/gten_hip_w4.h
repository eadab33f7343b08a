/* gten_hip_w4.h -- GPTQ and AWQ 4-bit checkpoint tensors (qweight / qzeros / scales, optionally g_idx) unpacked, TRANSPOSED and
 * dequantised ON THE DEVICE while they are quantised and packed (csrc/gten_quant_w4.h).
 *
 * Our weight is [rows = N out features][cols = K in features]; these checkpoints store [in features][out features], contiguous
 * along the output feature.  The call writes, in ONE launch and without a dense copy in HBM or on the host, the bytes
 *     the packed weight of convert.quantize(D, dst_dtype, "f16")      (GTEN_Q8 / GTEN_Q4; the block delta rounded to f16)
 *     the dense rows of D                                              (GTEN_F16)
 * for the f16 matrix
 *     D(n, k) = to_f16((float)(q(k, n) - z(g(k), n)) * widen(scales[g(k)][n]))        one f32 product (exact), one rounding to f16
 * tests/w4_ref.py restates it in NumPy.  4 bits only.  G = cols / group_size groups, or 1 for group_size = -1.  All little-endian.
 * The table shapes and nibble positions are written down from the public AutoGPTQ / AutoAWQ (GEMM) formats; no trained
 * checkpoint was at hand to compare them with.
 *
 *   GTEN_W4_GPTQ (0)   qweight int32 [K/8][N]   qzeros int32 [G][N/8]   scales f16 [G][N]   g_idx int32 [K] or NULL
 *       q(k, n) = (qweight[k >> 3][n] >> 4 (k & 7)) & 15
 *       g(k)    = g_idx ? g_idx[k] : k / group_size                      (group_size -1: 0)
 *       z(g, n) = ((qzeros[g][n >> 3] >> 4 (n & 7)) & 15) + zero_offset   zero_offset 1 for checkpoint_format gptq, 0 for gptq_v2;
 *                                                                        nothing wraps: z may be 16
 *   GTEN_W4_AWQ (1)    qweight int32 [K][N/8]   qzeros int32 [G][N/8]   scales f16 [G][N]   no g_idx, zero_offset 0
 *       column 8 c + j sits at nibble position P[j], P = {0, 4, 1, 5, 2, 6, 3, 7}
 *       q(k, n) = (qweight[k][n >> 3] >> 4 P[n & 7]) & 15
 *       z(g, n) = (qzeros[g][n >> 3] >> 4 P[n & 7]) & 15
 *       g(k)    = k / group_size
 *
 * Refused: cols % 32, rows % 8, a group_size that is neither -1 nor a multiple of 32 that divides cols; a g_idx entry outside
 * [0, G) (named; the kernel never indexes with it); an infinite or NaN D (an infinite scale), as by every quantising call. */
#ifndef GTEN_HIP_W4_H
#define GTEN_HIP_W4_H
#include "gten_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { GTEN_W4_GPTQ = 0, GTEN_W4_AWQ = 1 };

/* bytes of one of the four tensors of a [rows = N][cols = K] weight: which 0 qweight, 1 qzeros, 2 scales, 3 g_idx (0 for AWQ, which
 * has none); 0 for a bad argument (a layout or `which` out of range, or a shape / group_size the call below refuses) */
size_t gten_hip_w4_src_bytes(int layout, int which, int rows, int cols, int group_size);

/* qweight, qzeros, scales, g_idx (or NULL: g(k) = k / group_size): device memory, 16-byte aligned.  dst_packed: rows *
 * gten_hip_row_bytes(dst_dtype, cols) bytes, the packed weight layout of gten_hip.h (GTEN_Q8 / GTEN_Q4) or dense f16 rows
 * (GTEN_F16), 16-byte aligned.  zero_offset: 0 or 1 (AWQ: 0).  Queued on the selected stream, then waited for (the non-finite and
 * g_idx flags are read back).  Like every writer it announces its output range. */
int gten_hip_quantize_weight_w4(const void* qweight, const void* qzeros, const void* scales, const void* g_idx, int layout, int zero_offset,
                                int rows, int cols, int group_size, int dst_dtype, void* dst_packed);

#ifdef __cplusplus
}
#endif
#endif
