/*
 * gten_host_prefix.h -- a prefix that the prompts of a batch share, at the model level (libgten_host.so,
 * host/capi_prefix.cpp), beside include/gten_host.h.  DESIGN.md §3.9.
 *
 * While a prefix of P ids is set, a prompt whose first P ids equal it and that has at least 16 ids after them is processed
 * the short way by gten_host_batch_prefill, _prefill_many, _generate, _generate_topk, _serve, _serve2 and _serve_topk: only
 * the ids after the prefix go through the model (include/gten_hip_prefix.h), and the slot's caches receive a copy of the
 * prefix's K / V rows in front of theirs.  Logits, ids and cache bytes are those of processing the prompt whole.  Every
 * other prompt -- no match, fewer than 16 ids of its own -- goes exactly as without a prefix.  Host pointers throughout.
 */
#ifndef GTEN_HOST_PREFIX_H
#define GTEN_HOST_PREFIX_H

#include <stdint.h>

#include "gten_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The ids every later prompt of this batch may begin with (n = 0: none).  Processed ONCE, as one segment, onto a cache set of
 * its own; 16 <= n, n + 17 <= max_ctx.  -2 when the batch does not process prompts as segments (fewer than 16 sequences, or
 * gten_hip_row_segments_ok says no); < 0 on bad arguments.  Replacing the prefix does not disturb sequences in flight. */
int gten_host_batch_set_prefix(gten_host_batch* b, const int32_t* tokens, int n);
/* the prefix's length; prompts that took the short way so far; prompt rows computed so far in segmented calls (both ways;
 * the prefix's own rows are not counted).  Any of the three may be NULL. */
int gten_host_batch_prefix_info(gten_host_batch* b, int* n_prefix, unsigned long long* prompts_shared, unsigned long long* rows_computed);

#ifdef __cplusplus
}
#endif

#endif
