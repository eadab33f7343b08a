/*
 * gten_host_sessions.h -- continuing sequences instead of recomputing them, exported by libgten_host.so beside
 * include/gten_host.h (host/capi_sessions.cpp).  DESIGN.md §3.17.
 *
 * gten_host_batch_prefill and _prefill_many process a prompt from position 0.  A conversation's next turn needs only its new
 * rows: the sequence's caches keep rows [0, ctx) and the turn's ids become positions ctx ..  (include/gten_hip_continue.h:
 * several sequences' new rows are ONE row matrix, each segment behind its own cache rows).  Logits and cache bytes are those
 * of processing history + turn whole, where the kept rows came from the prompt path; rows that decode steps wrote differ
 * from the prompt path's inside the decode path's band.  Sessions keep such a sequence -- a cache set of its own, the history,
 * its valid rows -- between serving calls, and gten_host_batch_serve_sessions serves their turns.  Host pointers throughout.
 */
#ifndef GTEN_HOST_SESSIONS_H
#define GTEN_HOST_SESSIONS_H

#include <stdint.h>

#include "gten_host.h"
#include "gten_host_fsm.h"

#define GTEN_HOST_SESSIONS_MAX 256

#ifdef __cplusplus
extern "C" {
#endif

/* Sequence seqs[k] keeps rows [0, ctx_len[k]) of its caches; segment k = tokens[starts[k] .. starts[k + 1]) (>= 1 id) becomes
 * positions ctx_len[k] ...  Where the batch processes prompts as segments, the segments share row matrices (at most 32
 * segments / 4096 rows each, formed in order); one of fewer than 16 ids is filled up to 16 rows behind its last id -- rows do
 * not depend on later rows, the fill is computed and dropped -- so that it, too, leaves the whole prompt's bytes.  A
 * conversation of fewer than 16 ids in all (ctx_len + ids: a prompt that short goes through the operators), a filled segment
 * that would end past position 2048, and every segment of other batches go one by one through the sequence's own model
 * object.  logits_out, when given, is [n][n_vocab]: the logits of each segment's last row; first_out,
 * when given, their argmax (first maximum).  -1: a sequence out of range or repeated, ctx_len < 1, an empty segment,
 * ctx_len + ids > max_ctx. */
int gten_host_batch_extend_many(gten_host_batch* b, const int32_t* seqs, const int32_t* ctx_len, const int32_t* tokens, const int32_t* starts, int n,
                                float* logits_out, int32_t* first_out);
/* since the batch was made: segments that went as continued row matrices, the rows computed for them, the context rows they
 * kept (= rows not recomputed), the rows of segments that went one by one.  Any may be NULL. */
int gten_host_batch_extend_info(gten_host_batch* b, unsigned long long* turns_continued, unsigned long long* rows_computed,
                                unsigned long long* rows_kept, unsigned long long* rows_one_by_one);

/* The rows a conversation's next turn computes (host/session_plan.h; no device involved): n_ids ids of history with `rows`
 * leading valid K / V rows, n_new more ids; `segmented` != 0: prompts are processed as segments.  ctx = min(rows,
 * n_ids + n_new - 1) rows are kept, compute = n_ids + n_new - ctx >= 1 rows computed; path 0: the whole prompt (ctx 0), 1: a
 * continued segment (n_ids + n_new >= 16 and segmented; of max(compute, 16) matrix rows), 2: one by one.  Any out pointer may be NULL.  -1: negative counts,
 * rows > n_ids, or n_ids + n_new < 1. */
int gten_host_session_plan(int n_ids, int rows, int n_new, int segmented, int* ctx, int* compute, int* path);

/* ---- Sessions: a conversation that keeps its K / V between serving calls.  A session owns a cache set of its own (what a
 * spare set of the serving queue costs), `ids` -- the history -- and `rows`, the leading positions that have valid K / V.
 * Room for n sessions in all (at most GTEN_HOST_SESSIONS_MAX; never shrinks); -1 outside that. */
int gten_host_batch_sessions_reserve(gten_host_batch* b, int n);
/* a new, empty session: its id (>= 0), or -1 when every reserved one is open */
int gten_host_batch_session_open(gten_host_batch* b);
/* the session ends, its id may be handed out again; -1: not an open session */
int gten_host_batch_session_close(gten_host_batch* b, int id);
/* ids held, valid rows, and the prefix mark its set carries (the registered prefix -- include/gten_host_prefixes.h -- whose rows
 * its first turn copied, and how many; -1 / 0 without one: replacing that prefix, or a turn that keeps fewer rows, drops it).
 * Any out pointer may be NULL.  -1: not an open session. */
int gten_host_batch_session_info(gten_host_batch* b, int id, int* n_ids, int* rows, int* prefix_which, int* prefix_rows);
/* the first min(n, ids held) ids into out; returns how many the session holds, -1: not an open session */
int gten_host_batch_session_ids(gten_host_batch* b, int id, int32_t* out, int n);
/* the history is cut to its first n_ids ids, rows = min(rows, n_ids); nothing moves on the device.  How a caller regenerates or
 * edits the last turn.  -1: not an open session, n_ids outside [0, ids held]. */
int gten_host_batch_session_truncate(gten_host_batch* b, int id, int n_ids);
/* open sessions; K / V bytes of one session's set; session items served since the batch was made, those of them that went as
 * continued segments, the rows computed for session items and the rows kept (= not recomputed).  Any may be NULL. */
int gten_host_batch_sessions_info(gten_host_batch* b, int* open, unsigned long long* kv_bytes_per_session, unsigned long long* turns,
                                  unsigned long long* turns_continued, unsigned long long* rows_computed, unsigned long long* rows_kept);

/* gten_host_batch_serve_fsm (include/gten_host_fsm.h: the same arguments, the same meaning) with a session per item: session[j] =
 * -1 is that call's item, byte for byte; session[j] = s: prompts[j] holds only the turn's NEW ids (n_prompt[j] >= 0: an empty
 * turn regenerates behind a truncated history), and the item behaves in every respect -- limits, positions, the sampler's
 * position-keyed noise, the penalty window, the automaton's position, the out row, n_total, ended_by -- as the prompt
 * ids(s) + prompts[j], except for the rows that are computed (gten_host_session_plan).  Its cache set is the session's own; when
 * the item ends the session holds the out row, with rows = ids - 1 if it generated an id, else ids.  An item without room to
 * generate is returned as it is and leaves its session unchanged.  -1 as well: a session that is not open or named twice, a
 * history + turn that out's stride max(max_tokens, max_prompt) or the context does not hold. */
int gten_host_batch_serve_sessions(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int n_prompts, int max_prompt, int max_tokens,
                                   int eos, int slice, int max_new, const int32_t* max_new_each, int32_t* out, int32_t* n_total, double* stats, int n_stats,
                                   const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed, const int32_t* table,
                                   const int32_t* min_new, const int32_t* n_top, int n_top_max, float* logprob_out, int32_t* top_id_out,
                                   float* top_logprob_out, const float* top_p, const float* min_p, float top_p_all, float min_p_all,
                                   const gten_host_penalties* pen, const int32_t* fsm_start, int32_t* ended_by, const int32_t* session);

#ifdef __cplusplus
}
#endif

#endif
