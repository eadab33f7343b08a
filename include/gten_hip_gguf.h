/* gten_hip_gguf.h -- weights decoded from the ggml block stream of a GGUF tensor ON THE DEVICE while they are quantised and
 * packed (csrc/gten_quant_gguf.h).
 *
 * For a tensor of ggml type T the call writes, in ONE launch and without a dense copy in HBM or on the host, the bytes
 *     the packed weight of convert.quantize(D_T(blocks)[row map], dst_dtype, "f32")      (GTEN_Q8 / GTEN_Q4)
 *     to_f16(D_T(blocks)[row map])                                                        (GTEN_F16)
 * where D_T is ggml's own dequantisation in f32 -- every operation below ONE correctly rounded IEEE f32 operation, the f16 -> f32
 * widening of d / dmin and the integer -> f32 conversions exact -- and the quantiser is include/gten_hip_quant.h's with an f32
 * source.  tests/gguf_ref.py restates D_T in NumPy.  All fields little-endian; blocks of a row follow each other, rows follow
 * each other, nothing is padded: a row starts wherever its byte offset falls (2-byte aligned).
 *
 *   GTEN_GGML_Q8_0 (8)   34 B / 32 elements   { f16 d; i8 q[32] }
 *       x[j] = (float)q[j] * d
 *   GTEN_GGML_Q4_0 (2)   18 B / 32            { f16 d; u8 qs[16] }                           j in 0..15
 *       x[j] = (float)((qs[j] & 15) - 8) * d          x[j + 16] = (float)((qs[j] >> 4) - 8) * d
 *   GTEN_GGML_Q5_0 (6)   22 B / 32            { f16 d; u32 qh; u8 qs[16] }                   j in 0..15
 *       x[j]      = (float)(((qs[j] & 15) | (((qh >> j) & 1) << 4)) - 16) * d
 *       x[j + 16] = (float)(((qs[j] >> 4) | (((qh >> (j + 16)) & 1) << 4)) - 16) * d
 *   GTEN_GGML_Q4_K (12)  144 B / 256          { f16 d; f16 dmin; u8 sc[12]; u8 qs[128] }
 *       sub-block j in 0..7 (32 elements):  j < 4:  s = sc[j] & 63,                              m = sc[j + 4] & 63
 *                                           else:   s = (sc[j + 4] & 15) | ((sc[j - 4] >> 6) << 4),  m = (sc[j + 4] >> 4) | ((sc[j] >> 6) << 4)
 *       element l in 0..31 of sub-block j = 2 g + h:   q = (qs[32 g + l] >> 4 h) & 15
 *       x = ((d * (float)s) * (float)q) - (dmin * (float)m)          three products and one difference, each rounded
 *   GTEN_GGML_Q5_K (13)  176 B / 256          { f16 d; f16 dmin; u8 sc[12]; u8 qh[32]; u8 qs[128] }
 *       as Q4_K with   q = ((qs[32 g + l] >> 4 h) & 15) + 16 * ((qh[l] >> j) & 1)
 *   GTEN_GGML_Q6_K (14)  210 B / 256          { u8 ql[128]; u8 qh[64]; i8 sc[16]; f16 d }
 *       half n in 0..1, k in 0..3, l in 0..31:
 *       q = ((ql[64 n + 32 (k & 1) + l] >> 4 (k >> 1)) & 15) | (((qh[32 n + l] >> 2 k) & 3) << 4)
 *       x[128 n + 32 k + l] = (d * (float)sc[8 n + 2 k + l / 16]) * (float)(q - 32)
 *
 * ROW MAP.  llama.cpp's converter interleaves the rows of attn_q / attn_k per head.  With n_head > 0 and D = rows / n_head,
 * destination row h D + t (D / 2) + i  (t in {0, 1}, i < D / 2) is decoded from source row h D + 2 i + t: the Hugging Face order
 * the operators expect.  n_head = 0: the identity.
 *
 * A decoded NaN or infinity is outside the definition: the call fails (the message names it) and the destination is unspecified. */
#ifndef GTEN_HIP_GGUF_H
#define GTEN_HIP_GGUF_H
#include "gten_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ggml type codes of the block formats above */
enum { GTEN_GGML_Q4_0 = 2, GTEN_GGML_Q5_0 = 6, GTEN_GGML_Q8_0 = 8, GTEN_GGML_Q4_K = 12, GTEN_GGML_Q5_K = 13, GTEN_GGML_Q6_K = 14 };

/* bytes of the block stream of a [rows][cols] tensor; 0 for a type that is not one of the six, for rows or cols <= 0 and for
 * cols that are no multiple of the format's block (256 for the K formats, 32 for the others) */
size_t gten_hip_gguf_src_bytes(int ggml_type, int rows, int cols);

/* blocks: the block stream in device memory, 16-byte aligned;  dst_packed: rows * gten_hip_row_bytes(dst_dtype, cols) bytes, the
 * packed weight layout of gten_hip.h (GTEN_Q8 / GTEN_Q4) or dense f16 rows (GTEN_F16), 16-byte aligned.  n_head: the row map
 * (0, or a divisor of rows that leaves an even D).  Queued on the selected stream, then waited for (the non-finite flag is read
 * back).  Like every writer it announces its output range. */
int gten_hip_quantize_weight_gguf(const void* blocks, int ggml_type, int rows, int cols, int n_head, int dst_dtype, void* dst_packed);

#ifdef __cplusplus
}
#endif
#endif
