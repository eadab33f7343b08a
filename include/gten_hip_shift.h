/*
 * gten_hip_shift.h -- context shift: drop rows [keep, keep + drop) of a sequence's K / V caches, slide the rows behind them down
 * and rotate every moved K row back by `drop` positions, in place; exported by libgten_hip.so beside include/gten_hip_beam.h
 * (same conventions: device pointers unless the name ends in _host, 0 on success, otherwise a code with gten_hip_last_error()).
 * DESIGN.md §3.20.
 *
 * shift(keep, drop) acts on a cache whose rows [0, n) are valid, 0 <= keep, 1 <= drop, keep + drop <= n.  m = n - keep - drop rows
 * move:
 *   V  row keep + i becomes the bytes of the old row keep + drop + i, i in [0, m);
 *   K  row keep + i becomes unrot(old row keep + drop + i, drop), where unrot(row, d) is
 *        1. swap the two halves of every head of the stored row (f16: half-words j and j + d_head / 2; Q8, d_head 64: the head's
 *           two 34-byte blocks, whole; Q8, d_head 32: the two 16-quant halves inside the block, which share one delta),
 *        2. gten_hip_rotary_emb at row index d,
 *        3. swap the halves back
 *      -- the rotation by minus d: v0' = v0 * c + v1 * s, v1' = v1 * c - v0 * s with (c, s) the RoPE table's entry (d, j), every f32
 *      operation rounded on its own, the row read and written in the activation dtype with the library's quantiser;
 *   rows [0, keep), rows [keep + m, ...) and the pitch padding keep their bytes: nothing outside [keep, keep + m) is written.
 * The cache then has n - drop valid rows.  After a shift the caches are NOT what recomputing the shortened text would give: the kept
 * rows were computed while attending to the dropped ones, and each moved K element carries one more rounding per shift.
 */
#ifndef GTEN_HIP_SHIFT_H
#define GTEN_HIP_SHIFT_H

#include <stddef.h>
#include <stdint.h>

#include "gten_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one (sequence, layer): its K and V caches (device, row r at r * pitch) and the shift */
typedef struct { void* k; void* v; int32_t n, keep, drop; } gten_hip_kv_shift_item;

/* activation dtype Q8 or F16, d_head 32 or 64, kv_dim % d_head == 0; every item must be valid (0 <= keep, 1 <= drop,
   keep + drop <= n <= 2048); there is no no-op form.  `items_host`: host array.  All items go in one launch on the current stream
   (one more per 65535 items); a call that is refused has written nothing.  Every item's rows [keep, keep + m) of K and V are
   announced to the watched caches (head-major shadows, shared prefix copies) like any other write. */
int gten_hip_kv_shift(const gten_hip_kv_shift_item* items_host, int n_items, int adtype, size_t pitch, int kv_dim, int d_head);

#ifdef __cplusplus
}
#endif

#endif
