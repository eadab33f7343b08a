/*
 * gten_hip_continue.h -- prompt rows that CONTINUE CONTEXTS OF THEIR OWN, exported by libgten_hip.so beside include/gten_hip.h
 * (same conventions: device pointers, 0 on success, otherwise a code with gten_hip_last_error()).  DESIGN.md §3.17.
 *
 * include/gten_hip_prefix.h puts every segment of a row matrix behind ONE prefix.  A batch of continued conversations has a
 * context per segment: segment s's rows are positions len_s + 0 .. and read positions [0, len_s) from that segment's own
 * K / V rows (a cache set's tensors).  RoPE and the attention are still one launch each for all segments: the rotation
 * takes a row's position from its segment's record, the attention takes start position, context pointers and the shift of
 * its base pointers per workgroup from the row tile's segment.
 */
#ifndef GTEN_HIP_CONTINUE_H
#define GTEN_HIP_CONTINUE_H

#include <stdint.h>

#include "gten_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* K / V rows [0, len) of one segment's context on one layer: activation dtype, the caches' pitch, 16-byte aligned, read only */
typedef struct { const void* k; const void* v; int32_t len; } gten_hip_row_ctx;

/* The contexts of the row segments that are set (gten_hip_set_row_segments), for every layer of a prompt batch:
 * ctx[layer * n_segments + s].  n_segments must be the number of segments set; len >= 1, len + the segment's rows <= 2048,
 * and a segment's len is the same on every layer.  The records go to the device ONCE, on the calling stream, together with
 * the row tiles (ordered by the positions a tile really walks, len + its last row, longest first) and the rows' positions;
 * the block calls of the batch then wait for nothing on the host.  NULL / 0 clears.  EVERY call of gten_hip_set_row_segments,
 * one with equal values included, ends the contexts' validity: gten_hip_block_rows_continued refuses until they are set again
 * (so a caller cannot run on the K / V pointers of an earlier batch by setting the same segments). */
int gten_hip_set_row_contexts(const gten_hip_row_ctx* ctx, int n_layers, int n_segments);

/* gten_hip_block_rows for rows that continue the contexts of `layer` (0 <= layer < n_layers of the set call).  Every buffer of
 * the descriptor ends with the bytes that gten_hip_block_rows_prefixed leaves when it is called for segment s alone with
 * (k_s, v_s, len_s).  GTEN_HIP_NOT_HANDLED exactly where gten_hip_block_rows answers it. */
int gten_hip_block_rows_continued(const gten_hip_block_desc* b, int n, int layer);

#ifdef __cplusplus
}
#endif

#endif
