/* gten_hip_quant.h -- weights quantised and packed ON THE DEVICE from dense f32 / bf16 / f16 rows (DESIGN.md 3.26;
 * csrc/gten_quant.h).
 *
 * gten_hip_pack_weight (gten_hip.h) takes a block stream that was quantised on the CPU.  gten_hip_quantize_weight takes the
 * unquantised matrix and writes, in ONE launch and without an intermediate block stream, the bytes
 *     gten_hip_pack_weight(convert.quantize(w, dst_dtype, src_dtype))
 * would leave (tinyllama.cpp_amd/convert.py is the definition; w = the f32 widening of the source).  Per block of 32:
 *     amax    = max |x|
 *     delta32 = round_to_src(amax / qmax)         f32 IEEE division, then round-to-nearest-even to bf16 / f16 for a bf16 / f16
 *                                                 source; qmax = 127 (Q8), 7 (Q4)
 *     scale   = delta32 != 0 ? 1.0f / delta32 : 0
 *     q       = rint(x * scale)                   one f32 multiply, half to even; then the int32 conversion of NumPy on x86
 *     stored delta = f16(delta32)                 may be 0, subnormal or infinite
 *     Q8 byte = q & 0xff;   Q4 byte j = (((q[j] + 7) << 4) | (q[j + 16] + 7)) & 0xff
 * A GTEN_F16 destination is the row rounded to f16 (nearest even, overflow to infinity).
 * NON-FINITE source values are outside the definition: the call fails (the message names it) and the destination is
 * unspecified. */
#ifndef GTEN_HIP_QUANT_H
#define GTEN_HIP_QUANT_H
#include "gten_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* source dtype codes; bf16 is the raw upper 16 bits of an f32 */
enum { GTEN_HIP_SRC_F32 = 0, GTEN_HIP_SRC_BF16 = 1, GTEN_HIP_SRC_F16 = 2 };

/* bytes of a dense [rows][cols] matrix in a source dtype (0 for a bad code or shape) */
size_t gten_hip_quant_src_bytes(int src_dtype, int rows, int cols);

/* src_rows: dense [rows][cols] in src_dtype, device memory, 16-byte aligned;  dst_packed: rows * gten_hip_row_bytes(dst_dtype,
 * cols) bytes in the packed weight layout of gten_hip.h (GTEN_Q8 / GTEN_Q4, cols % 32 == 0) or dense f16 rows (GTEN_F16),
 * 16-byte aligned.  Queued on the selected stream, then waited for (the non-finite flag is read back).  Like every writer it
 * announces its output range. */
int gten_hip_quantize_weight(const void* src_rows, int src_dtype, int rows, int cols, int dst_dtype, void* dst_packed);

#ifdef __cplusplus
}
#endif
#endif
