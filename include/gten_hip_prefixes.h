/*
 * gten_hip_prefixes.h -- SEVERAL shared prompt prefixes per decoder, exported by libgten_hip.so beside
 * include/gten_hip_prefix_decode.h (same conventions: device pointers, 0 on success, otherwise a code with
 * gten_hip_last_error()).  DESIGN.md section 3.9, "several prefixes".
 */
#ifndef GTEN_HIP_PREFIXES_H
#define GTEN_HIP_PREFIXES_H

#include <stdint.h>

#include "gten_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* prefix indices are 0 .. GTEN_PREFIXES_MAX - 1; index 0 is the prefix of include/gten_hip_prefix_decode.h */
#define GTEN_PREFIXES_MAX 8

/*
 * A decoder that keeps head-major shadows holds up to GTEN_PREFIXES_MAX prefix shadows at the same time, each laid out as a
 * sequence's and allocated on the first use of its index.  A sequence shares AT MOST ONE of them.  What
 * include/gten_hip_prefix_decode.h says about one prefix holds for every index on its own: every prefix has its own watch on
 * its set's rows, its own "shadow is stale" state and its own import count, and whatever ends a promise there ends it here.
 * gten_hip_decoder_prefix_set(dec, kv, len) IS prefixes_set(dec, 0, kv, len), gten_hip_decoder_slot_share(dec, seq, rows) IS
 * prefixes_share(dec, seq, 0, rows).  On a decoder without shadows every call below succeeds and does nothing (info reports
 * -1 / 0).
 *
 * prefixes_set: as prefix_set, for index `which` (kv = NULL or prefix_len = 0 clears it).  Only the sequences that share
 * prefix `which` are taken off it (count 0, their own shadows imported in full from their own rows before their next step,
 * and before shadow `which` is imported again); sequences behind other prefixes keep their chunks and are not imported.  So
 * does a write into the rows of prefix `which`'s set that is announced to this library.  The FIRST call with which >= 1 that
 * sets a prefix drops the decoder's captured graphs once more: from then on its step launches the attention instantiations
 * that pick a sequence's shadow from a table (_pfxn); a decoder that only ever used index 0 launches what it launched before
 * this header existed.
 */
int gten_hip_decoder_prefixes_set(gten_hip_decoder* dec, int which, const gten_hip_kv_ptrs* kv, int prefix_len);
/* prefixes_share: slot_share's promise and refusals, judged against prefix `which` (refused as well: which outside
 * [0, GTEN_PREFIXES_MAX), an index that is not set).  A new promise replaces the sequence's old one, whichever prefix that
 * spoke of; rows = 0 withdraws whatever promise the sequence has. */
int gten_hip_decoder_prefixes_share(gten_hip_decoder* dec, int seq, int which, int rows);
/* prefixes_info: the prefix sequence seq's next step shares (seq_which; -1: none) and the chunks it reads from that shadow;
 * for prefix `which`: its length (0: not set), the imports of its shadow so far, the sequences that share it now.  Any out
 * pointer may be NULL. */
int gten_hip_decoder_prefixes_info(gten_hip_decoder* dec, int seq, int which, int* seq_which, int* seq_chunks, int* prefix_len,
                                   unsigned long long* prefix_imports, int* sharers);

#ifdef __cplusplus
}
#endif

#endif
