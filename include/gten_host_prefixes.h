/*
 * gten_host_prefixes.h -- SEVERAL shared prompt prefixes per batch at the model level (libgten_host.so,
 * host/capi_prefixes.cpp), beside include/gten_host_prefix.h and include/gten_host_prefix_decode.h.  DESIGN.md section 3.9,
 * "several prefixes".
 *
 * A batch holds up to 8 prefixes at the same time, index `which` = 0 .. 7 (GTEN_PREFIXES_MAX of include/gten_hip_prefixes.h),
 * each processed once onto a cache set of its own.  A later prompt takes the LONGEST registered prefix it begins with and has
 * at least 16 ids behind (gten_host_prefixes_match): only its own rows are computed, its cache set gets a copy of that
 * prefix's K / V rows in front, and the sequence or serving slot that decodes on the set reads the prefix's full chunks of 256
 * positions from the shared decoder's one copy of THAT prefix.  Ids, logits and cache rows are the bytes of processing every
 * prompt whole and decoding on private copies.  Index 0 is the prefix of gten_host_batch_set_prefix: that call and
 * gten_host_batch_prefix_info go on meaning what they meant and speak of index 0.  Prefixes are independent: a prefix that
 * begins with another registered one is stored in full beside it.
 */
#ifndef GTEN_HOST_PREFIXES_H
#define GTEN_HOST_PREFIXES_H

#include <stdint.h>

#include "gten_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gten_host_batch_set_prefix at index `which`: 16 <= n and n + 17 <= context; n = 0 clears the index.  0; -1: bad arguments
 * (which outside 0 .. 7 among them); -2: this batch does not process prompts as segments (up to 8 sequences, other head
 * shapes).  Replacing or clearing prefix `which` disturbs neither the sequences in flight (those that decode behind it go back
 * to their own copies of its rows first) nor the cache sets and slots behind OTHER prefixes. */
int gten_host_batch_prefixes_set(gten_host_batch* b, int which, const int32_t* tokens, int n);
/* per prefix: its length (0: none), the prompts that took the short way behind it so far and the rows computed for them.
 * Any out pointer may be NULL. */
int gten_host_batch_prefixes_info(gten_host_batch* b, int which, int* n_prefix, unsigned long long* prompts_shared,
                                  unsigned long long* rows_computed);
/* the shared decoder's view (gten_hip_decoder_prefixes_info): the prefix index sequence / slot `seq` shares at its next step
 * (which_out; -1: none) and the leading chunks it reads from that one copy; for prefix `which`: the length the decoder holds,
 * the imports of its copy so far, the sequences sharing it now.  Any out pointer may be NULL. */
int gten_host_batch_prefixes_decode_info(gten_host_batch* b, int seq, int* which_out, int* chunks_out, int which, int* n_prefix,
                                         unsigned long long* prefix_imports, int* sharers);
/* gten_hip_decoder_prefixes_share on the batch's decoder, its return code passed on (0; not 0: refused, the message is
 * gten_hip_last_error()); the batch makes these calls itself -- for callers that fill caches themselves, and tests */
int gten_host_batch_prefixes_decode_share(gten_host_batch* b, int seq, int which, int rows);
/* Tests: prefix `which`'s own single-sequence decoder decodes steps n_first .. n_first + steps - 1 over tokens[0, count) on
 * the prefix's cache set, i.e. REWRITES its rows from n_first - 1 on (as gten_host_batch_seq_steps does with a sequence's).
 * The registration at `which` ends on the batch's side (the set no longer holds those ids); the shared decoder is told
 * nothing and hears of the write through its watch.  -1: bad arguments or nothing registered at `which`. */
int gten_host_batch_prefixes_steps(gten_host_batch* b, int which, const int32_t* tokens, int count, int n_first, int steps);
/* no batch, no device: prefix i (i < n_prefixes <= 64) is prefix_ids[i * max_len .. i * max_len + lens[i]), lens[i] = 0: not
 * registered.  The index of the longest prefix that prompt[0, n) begins with and has at least 16 ids behind; of two such
 * prefixes of the same length (they hold the same ids) the lower index; -1: none. */
int gten_host_prefixes_match(const int32_t* prefix_ids, const int* lens, int n_prefixes, int max_len, const int32_t* prompt, int n);

#ifdef __cplusplus
}
#endif

#endif
