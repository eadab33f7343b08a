/* gten_hip_lora.h -- a LoRA adapter merged into a weight matrix WHILE it is quantised and packed on the device (DESIGN.md 3.27;
 * csrc/gten_quant_lora.h).  The unmerged form of the call is in gten_hip_quant.h, whose source dtype codes
 * (GTEN_HIP_SRC_F32 / _BF16 / _F16) this header uses for the matrix and for the adapter.
 *
 * For a source matrix w [rows][cols], adapter matrices A [rank][cols] and B [rows][rank] (the PEFT layout: lora_A.weight,
 * lora_B.weight) and an f32 scale (lora_alpha / r), every element widened to f32 and every step ONE correctly rounded f32
 * operation (no fused multiply-add):
 *     acc = +0.0f
 *     for k = 0 .. rank-1, ascending:   acc = acc + (B[i][k] * A[k][j])
 *     m[i][j] = round_to_src( w[i][j] + (scale * acc) )        rounded to the SOURCE dtype: merged in the checkpoint's dtype
 * and the destination holds the bytes the unmerged call leaves for a source that already held m (for GTEN_F16: f16(m)).
 * tests/lora_ref.py restates this in NumPy.  The order of the sum is part of the definition.
 * A NON-FINITE m -- every NaN or infinity in w, A or B reaches one, and so does an overflow of the source dtype -- fails the
 * call (the message names it) and leaves the destination unspecified.
 * With scale == 0, or B all zeros (PEFT's initial state), m = w + 0: the bytes of the unmerged call, except that a negative zero
 * of the source becomes +0, which only a GTEN_F16 destination can show (a quant of -0 is 0 either way). */
#ifndef GTEN_HIP_LORA_H
#define GTEN_HIP_LORA_H
#include "gten_hip_quant.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { GTEN_HIP_LORA_MAX_RANK = 64 };

/* src_rows, dst_packed, rows, cols, src_dtype, dst_dtype: as in the unmerged call, with its checks; here cols % 8 == 0 for a
 * GTEN_F16 destination too (the rows of A keep the base's alignment).  a: dense [rank][cols], b: dense [rows][rank], both in
 * ab_dtype, device memory, 16-byte aligned at the base (B's rows need no alignment of their own).  Refused before any launch:
 * rank outside 1..GTEN_HIP_LORA_MAX_RANK, a scale that is not finite, a bad ab_dtype, a misaligned a or b.  Queued on the
 * selected stream, then waited for (the non-finite flag is read back); announces its output range like every writer. */
int gten_hip_quantize_weight_lora(const void* src_rows, int src_dtype, int rows, int cols,
                                  const void* a, const void* b, int rank, int ab_dtype, float scale,
                                  int dst_dtype, void* dst_packed);

#ifdef __cplusplus
}
#endif
#endif
