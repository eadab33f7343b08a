/* gten_hip_calib.h -- calibrated Q4 quantisation on the device: the importance of a weight's input columns
 * collected from activation rows (csrc/gten_col_energy.h), and a Q4 quantiser that picks every block's delta and quants among
 * 17 candidates by importance-weighted squared error (csrc/gten_quant_search.h).  The block format is gten_hip_quant.h's: the
 * same 18-byte blocks, quants in [-7, 7], so every Q4 kernel reads the result as it stands.  Source dtype codes
 * (GTEN_HIP_SRC_F32 / _BF16 / _F16) are that header's.
 *
 * THE SEARCH, operation by operation (every f32 operation rounded on its own, no fused multiply-add, no reassociation;
 * tests/calib_ref.py restates it in NumPy).  For the block of row r at columns c0 .. c0 + 31: x_j the f32 widening of the source,
 * w_j = importance[c0 + j] (1.0f everywhere for a null importance), amax = max |x_j|.
 *   S(t), the block sum of 32 f32 terms:   p_k = (((0 + t_8k) + t_8k+1) + ... + t_8k+7),  k = 0..3;   S = (p_0 + p_1) + (p_2 + p_3)
 *   err(d, q) = S( w_j * (e_j * e_j) ),  e_j = x_j - d * (float)q_j,  d an f16 value widened to f32
 *   candidate 0    the block gten_hip_quantize_weight writes: delta0 = f16(round_to_src(amax / 7)), q0_j = rint(x_j * scale).  It is
 *                  kept without a search when amax == 0 or delta0 is zero or not finite.
 *   candidate c, c = 1 .. 16:   is_c = (7.0f + 0.125f * (float)(c - 7)) / amax          (numerators 6.25 .. 8.125, exact)
 *                  q_j = clamp(rint(x_j * is_c), -7, 7);   A = S( w_j * (x_j * (float)q_j) );   B = S( w_j * ((float)q_j * (float)q_j) )
 *                  d_c = f16(A / B), round to nearest even;  valid when B > 0 and d_c is finite and not zero
 *   choice         c ascending from candidate 0; a valid candidate replaces the best so far when its err is strictly smaller, so
 *                  ties go to the lowest c and candidate 0 stays unless something is strictly better
 *   bytes          the chosen delta as f16 and byte j = ((q_j + 7) << 4) | (q_j+16 + 7), in the packed plane layout
 *                  gten_hip_pack_weight leaves */
#ifndef GTEN_HIP_CALIB_H
#define GTEN_HIP_CALIB_H
#include "gten_hip_quant.h"

#ifdef __cplusplus
extern "C" {
#endif

/* src_rows, src_dtype, rows, cols, dst_packed: as in gten_hip_quantize_weight with a GTEN_Q4 destination (Q8 gains nothing
 * measurable from a search and has none).  importance: f32 [cols] in device memory, 16-byte aligned, or null.
 * Refused before any launch: cols % 32 != 0, a misaligned pointer.  Refused by the kernel's flag words, each by name, with the
 * destination left unspecified: a NaN or an infinity in the source; an importance value that is negative, NaN or infinite.
 * Queued on the selected stream, then waited for (the flags are read back); announces its output range like every writer. */
int gten_hip_quantize_weight_search(const void* src_rows, int src_dtype, int rows, int cols,
                                    const float* importance, void* dst_packed);

/* acc[c] += sum over rows r = 0 .. n_rows-1 of (double)(v * v), v the f32 value of element c of row r and the square ONE f32
 * multiply.  rows: a row view as in gten_hip.h (row r at rows + r * pitch; base and pitch multiples of 2) of adtype GTEN_Q8
 * (v = (float)delta * (float)q of the row's 34-byte blocks) or GTEN_F16 (v the widening); cols a multiple of 32; acc: f64 [cols]
 * in device memory, 8-byte aligned.  Deterministic, no atomics: the rows are summed in chunks of 64 in ascending order, each
 * chunk from +0, and the chunk sums are added to acc in ascending order -- the same calls in the same order give the same bits.
 * Queued on the selected stream; announces acc as written. */
int gten_hip_calib_col_energy(const void* rows, int adtype, int n_rows, int cols, long long pitch, double* acc);

#ifdef __cplusplus
}
#endif
#endif
