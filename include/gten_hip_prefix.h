/*
 * gten_hip_prefix.h -- prompt rows that continue a SHARED PREFIX, exported by libgten_hip.so beside include/gten_hip.h
 * (same conventions: device pointers, 0 on success, otherwise a code with gten_hip_last_error()).  DESIGN.md §3.9.
 *
 * Several prompts that begin with the same ids need those ids' K / V rows once.  The caller processes the prefix alone
 * (one segment through gten_hip_block_rows), keeps every layer's K / V rows [0, prefix_len), and then processes only what
 * follows the prefix in each prompt: one row matrix whose segments are the prompts' remaining rows.  RoPE is one launch
 * over all of them (row r of segment k at position prefix_len + r - starts[k]) and so is the attention: positions
 * [0, prefix_len) are read from the shared prefix rows, later ones from the segment's own rows of the matrix.
 */
#ifndef GTEN_HIP_PREFIX_H
#define GTEN_HIP_PREFIX_H

#include <stdint.h>

#include "gten_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gten_hip_block_rows for rows that CONTINUE a shared prefix: row segments must be set; rows [starts[k], starts[k+1]) are
 * positions prefix_len + 0 .. of prompt k; k_prefix / v_prefix = the K / V rows [0, prefix_len) of this layer (activation
 * dtype, the caches' pitch).  Every buffer of the descriptor ends with the bytes that gten_hip_block_rows leaves in the
 * corresponding rows when each prompt is processed whole (prefix + its rows) as a segment.  prefix_len >= 1,
 * prefix_len + the longest segment <= 2048.  GTEN_HIP_NOT_HANDLED exactly where gten_hip_block_rows answers it. */
int gten_hip_block_rows_prefixed(const gten_hip_block_desc* b, int n, const void* k_prefix, const void* v_prefix, int prefix_len);

#ifdef __cplusplus
}
#endif

#endif
