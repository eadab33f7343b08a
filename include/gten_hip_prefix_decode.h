/*
 * gten_hip_prefix_decode.h -- decode slots that share a prompt PREFIX read one copy of its K / V, exported by libgten_hip.so
 * beside include/gten_hip.h and include/gten_hip_prefix.h (same conventions: device pointers, 0 on success, otherwise a code
 * with gten_hip_last_error()).  DESIGN.md section 3.9.
 */
#ifndef GTEN_HIP_PREFIX_DECODE_H
#define GTEN_HIP_PREFIX_DECODE_H

#include <stdint.h>

#include "gten_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * A decoder that keeps head-major shadows (gten_hip_set_kv_head_major; 16+ sequences, fast forms) can hold one more shadow, of
 * the rows [0, prefix_len) of a PREFIX cache set, and let sequences whose caches begin with those very rows read their leading
 * full chunks of 256 positions from it instead of from their own shadows: the decode attention's waves of all sharing
 * sequences then ask for the same lines and the chip's L2 serves them, and the import of a starting sequence skips those
 * chunks.  Per (sequence, head, chunk) the arithmetic is the same operations on the same bytes: ids and logits do not change.
 * On a decoder without shadows every call below succeeds and does nothing.
 *
 * prefix_set: kv[layer] (n_layers entries) are the prefix set's K / V caches -- whole caches of max_ctx rows in the decoder's
 * layout, of which rows [0, prefix_len) matter; they are watched like the sequences' own (a write into them through this
 * library takes every sequence off the shadow and re-imports it).  kv = NULL or prefix_len = 0 clears the prefix.  Either
 * way every sharing sequence is taken off the shadow FIRST (its count goes to 0 and its own shadow is imported in full from
 * its own rows before its next step) and only then is the prefix shadow imported again -- so the caller may overwrite the
 * prefix set's rows after a clearing call, or replace the prefix in place.  The first call that sets a prefix allocates the
 * shadow and drops the decoder's captured graphs (its step then launches the prefix-aware attention instantiations); a
 * decoder that never saw one launches exactly the kernels it always did. */
int gten_hip_decoder_prefix_set(gten_hip_decoder* dec, const gten_hip_kv_ptrs* kv, int prefix_len);
/* slot_share: the caller promises that rows [0, rows) of sequence seq's CURRENT cache set hold what the prefix set's rows hold
 * (rows = 0 withdraws the promise).  The sequence then reads floor(rows / 256) leading chunks from the prefix shadow.
 * Refused, nothing recorded: rows > prefix_len (or no prefix set); rows > n - 1 where n is the sequence's next step and the
 * decoder knows it -- a started slot, or outside the slot view a sequence that has been stepped and whose rows nobody has
 * written since.  Where it does not know (a parked slot, rows written since the last step), the sequence's next start names
 * the position and drops the promise if rows exceeds n - 1; so does every later (re)start or step call at such a position.
 * THE PROMISE ENDS with: gten_hip_decoder_slot_bind of the sequence (other caches); parking a started slot (slot_park,
 * slots_apply with n_first 0, entering the slot view); any write into the sequence's cache rows announced to this library
 * (every entry point that writes device memory; another decoder's appends) -- the sequence is then imported in full from its
 * rows, which stay the truth; any write into the prefix set's rows, and every prefix_set call.  A (re)start of the sequence
 * on the same caches at a position >= rows keeps it.  The decode appends go to the sequence's own rows and shadow only. */
int gten_hip_decoder_slot_share(gten_hip_decoder* dec, int seq, int rows);
/* the prefix length set (0: none), the chunks sequence seq's next step reads from the prefix shadow, imports of the prefix shadow
 * so far, and sequence imports that skipped shared chunks (any out pointer may be NULL) */
int gten_hip_decoder_prefix_info(gten_hip_decoder* dec, int seq, int* prefix_len, int* seq_chunks, unsigned long long* prefix_imports,
                                 unsigned long long* imports_skipping);
/* process-wide: slot_share records promises (on > 0, the default) or nothing (0: every sequence decodes on its own shadow);
 * on < 0 restores the default.  For tests and measurements: the same calls with the switch off are the reference side. */
int gten_hip_set_prefix_decode_shared(int on);


#ifdef __cplusplus
}
#endif

#endif
