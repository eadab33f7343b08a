/*
 * gten_hip_embed.h -- pooling the final-norm rows of several texts into one f32 vector per text on the device, exported by
 * libgten_hip.so beside include/gten_hip.h (same conventions: device pointers, 0 on success, otherwise a code < 0 with
 * gten_hip_last_error(); nothing is launched when an argument is refused).  Host side: include/gten_host_embed.h.
 * DESIGN.md §3.22.
 *
 * Input.  A row matrix in activation storage form (dtype GTEN_Q8: rows of 34-byte blocks {f16 delta, int8 q[32]}; GTEN_F16:
 * plain halfs), row r at x + r * pitch bytes, n_embd columns.  starts[0 .. n_segments] is a HOST table: segment k is rows
 * [starts[k], starts[k + 1]) and holds n = 1 .. GTEN_HIP_POOL_MAX_ROWS rows.  Output: f32 [n_segments][n_embd] on the device.
 *
 * The definition.  An exact statement in f32 / f64 arithmetic: it does not depend on the grid, on the wave, or on what else
 * is in the matrix.  A sum of several terms "in ascending order" starts from its first term and adds the others one by one,
 * every addition rounded to the format named.
 *   x[r][c]   the storage value as f32.  Q8: (float)q * f16_to_f32(delta), one f32 multiply.  f16: the conversion.
 *   GTEN_HIP_POOL_MEAN
 *     chunk j of a segment is its rows [64 j, min(64 j + 64, n));
 *     p_j[c]  = the f32 sum of the chunk's x[r][c], r ascending;
 *     s[c]    = the f32 sum of the p_j[c], j ascending;
 *     m[c]    = s[c] / (float)n, the division rounded to f32.
 *   GTEN_HIP_POOL_LAST
 *     m[c]    = x[n - 1][c].
 *   normalize != 0
 *     t[k]    = for k in 0 .. 63 the f64 sum of (double)m[c] * (double)m[c] over c = k, k + 64, ... ascending (every product
 *               is exact; no such c: 0);
 *     ss      = the f64 sum of t[0 .. 63], ascending;
 *     e[c]    = (float)((double)m[c] / sqrt(ss));   ss == 0 gives a row of +0.
 *   normalize == 0: the output is m.
 * NaN or +-inf among the values is outside the contract.
 *
 * Checks: x and out not null, dtype GTEN_Q8 or GTEN_F16, x and pitch multiples of 2, n_embd % 32 == 0 and 32 <= n_embd <=
 * GTEN_HIP_POOL_MAX_EMBD, pitch >= gten_hip_row_bytes(dtype, n_embd), 1 <= n_segments <= GTEN_HIP_POOL_MAX_SEGMENTS,
 * starts[0] >= 0, every segment 1 .. GTEN_HIP_POOL_MAX_ROWS rows, a known pooling.  Asynchronous, current stream.  Mean pooling
 * is two launches (the chunk sums into a scratch the library owns and grows on demand, one per stream; then one workgroup per
 * segment), last pooling one.  There is no floating-point atomic anywhere.
 */
#ifndef GTEN_HIP_EMBED_H
#define GTEN_HIP_EMBED_H

#include <stddef.h>
#include <stdint.h>

#include "gten_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GTEN_HIP_POOL_MEAN 0
#define GTEN_HIP_POOL_LAST 1
#define GTEN_HIP_POOL_MAX_SEGMENTS 32
#define GTEN_HIP_POOL_MAX_ROWS 2048
#define GTEN_HIP_POOL_MAX_EMBD 8192

int gten_hip_pool_rows(const void* x, int dtype, size_t pitch, int n_embd, const int32_t* starts, int n_segments, int pooling,
                       int normalize, float* out);

#ifdef __cplusplus
}
#endif
#endif
