/*
 * gten_hip_groups.h -- GROUP RECORDS of a decoder: snapshots of the leading K / V rows of one sequence that several sequences
 * read from ONE copy, exported by libgten_hip.so beside include/gten_hip_prefixes.h (same conventions: device pointers, 0 on
 * success, otherwise a code with gten_hip_last_error()).  DESIGN.md section 3.16.
 *
 * The samples of one prompt (include/gten_host_samples.h) agree on the whole prompt.  A decoder that keeps head-major shadows
 * holds, behind its GTEN_PREFIXES_MAX prefix records and in the same table, GTEN_GROUPS_MAX more records of the same kind: a
 * shadow laid out as a sequence's, allocated on the first use of its index, read by the _pfxn attention instantiations for the
 * leading full chunks of every sequence that shares it.  GTEN_PREFIXES_MAX stays 8 and every prefix call keeps its meaning; a
 * sequence that reads from a group record reports "no prefix" (-1, 0) through the prefix info calls.  A sequence shares ONE
 * record of either kind.  On a decoder without shadows every call below succeeds and does nothing (info reports -1 / 0).
 */
#ifndef GTEN_HIP_GROUPS_H
#define GTEN_HIP_GROUPS_H

#include <stdint.h>

#include "gten_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* group records are 0 .. GTEN_GROUPS_MAX - 1 (256 slots at four samples each) */
#define GTEN_GROUPS_MAX 64

/*
 * group_set: record g becomes a SNAPSHOT of rows [0, rows) of the caches kv[n_layers].  Its shadow is imported by the import
 * launch of the prefix shadows, queued by this call on the current stream -- which must be the stream the decoder's steps run
 * on.  THE CALLER GUARANTEES that the rows are visible to that stream and that nothing writes them before the queued import
 * has run.  Once the import is queued the record does not depend on the source rows: unlike a prefix it keeps NO WATCH, so a
 * later write into them, announced or not, does not concern it (the source is typically a sequence's own cache set, which is
 * overwritten with another prompt while its siblings still decode).  kv = NULL (or rows = 0) releases the record: the
 * sequences that share it come off first, exactly as prefixes_set takes them off (count 0, their own shadows imported in full
 * from their own rows before their next step).  The FIRST group_set of a decoder that sets a record switches its step to the
 * _pfxn attention instantiations and drops its captured graphs once -- the rule the first prefix index above 0 follows; a
 * decoder that never saw a group launches what it launched before this header existed.
 */
int gten_hip_decoder_group_set(gten_hip_decoder* dec, int g, const gten_hip_kv_ptrs* kv, int rows);
/* group_share: prefixes_share's promise -- "rows [0, rows) of sequence seq's OWN caches equal the snapshot" -- with the same
 * refusals, judged against record g (refused: g outside [0, GTEN_GROUPS_MAX), a record that is not set, rows beyond the
 * record, rows beyond the sequence's position).  It ends the way a prefix promise ends: a write into the sequence's rows,
 * slot_bind, parking a started slot.  A new promise replaces the sequence's old one of either kind; rows = 0 withdraws it.
 * With gten_hip_set_prefix_decode_shared(0) this call records nothing, too. */
int gten_hip_decoder_group_share(gten_hip_decoder* dec, int seq, int g, int rows);
/* groups_info: the record sequence seq's next step reads from (seq_group; -1: none) and the chunks it reads there; for record
 * g: its rows (0: not set), the imports of its shadow so far, the sequences that share it now.  Any out pointer may be NULL. */
int gten_hip_decoder_groups_info(gten_hip_decoder* dec, int seq, int g, int* seq_group, int* seq_chunks, int* rows,
                                 unsigned long long* imports, int* sharers);

#ifdef __cplusplus
}
#endif

#endif
