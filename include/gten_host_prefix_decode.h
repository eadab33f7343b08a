/*
 * gten_host_prefix_decode.h -- the decode side of a shared prefix at the model level (libgten_host.so, host/capi_prefix.cpp),
 * beside include/gten_host_prefix.h.  DESIGN.md section 3.9.
 *
 * gten_host_batch_set_prefix also hands the prefix's K / V rows to the batch's shared decoder
 * (include/gten_hip_prefix_decode.h).  A cache set that received a copy of them in front of a prompt's own rows -- every
 * prompt that took the short way -- is marked; the sequence or serving slot that decodes on it reads the prefix's full chunks
 * of 256 positions from the decoder's ONE copy.  This holds for prefill / prefill_many followed by the decode calls, for
 * generate, generate_topk, serve, serve2 and serve_topk; any later prompt onto the set (and gten_host_batch_seq_steps) clears
 * the mark.  Ids and logits are the same bytes as without it.  Batches whose decoder keeps no shadows (up to 8 sequences)
 * ignore all of it.
 */
#ifndef GTEN_HOST_PREFIX_DECODE_H
#define GTEN_HOST_PREFIX_DECODE_H

#include <stdint.h>

#include "gten_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the shared decoder's view (gten_hip_decoder_prefix_info): the prefix length it holds, the leading chunks sequence / slot
 * `seq` reads from the one copy at its next step, imports of that copy so far, and sequence imports that skipped shared
 * chunks so far.  Any out pointer may be NULL. */
int gten_host_batch_prefix_decode_info(gten_host_batch* b, int seq, int* n_prefix, int* seq_chunks, unsigned long long* prefix_imports,
                                       unsigned long long* imports_skipping);
/* gten_hip_decoder_slot_share on the batch's decoder, its return code passed on (0; not 0: refused, the message is
 * gten_hip_last_error()): the batch makes these calls itself; this one exists for callers that fill a sequence's caches
 * themselves, and for tests of the refusals */
int gten_host_batch_prefix_decode_share(gten_host_batch* b, int seq, int rows);
/* gten_hip_set_prefix_decode_shared: process-wide; > 0: on (the default), 0: no sequence shares from now on, < 0: the default again */
int gten_host_set_prefix_decode_shared(int on);

#ifdef __cplusplus
}
#endif

#endif
