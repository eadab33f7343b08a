/*
 * gten_host_samples.h -- n samples per prompt through the serving queue, exported by libgten_host.so beside
 * include/gten_host_fsm.h (same conventions).  DESIGN.md section 3.16.
 *
 * Prompt j is generated n_samples[j] times.  Sample i of prompt j is item e = first[j] + i of the EXPANDED queue, where
 * first[j] = n_samples[0] + .. + n_samples[j - 1]; it draws with item e's request and stream e.  Ids, ended_by, log-prob
 * records and n_total are, byte for byte, what gten_host_batch_serve_fsm returns for the expanded queue -- every prompt written
 * out n_samples[j] times in a row.  What differs is the price: a group's prompt is processed ONCE (the other members' cache
 * sets receive copies of the computed rows and draw their first ids from the one logits row), and -- with
 * gten_host_batch_set_groups_cap above 0 -- the members' decode slots read the prompt's full chunks of K / V from ONE copy, a group
 * record of the decoder (include/gten_hip_groups.h).  Nothing is
 * saved for prompts under 16 ids and on batches that do not process prompts as row segments (up to 8 sequences): there every
 * member runs as an ordinary item.
 */
#ifndef GTEN_HOST_SAMPLES_H
#define GTEN_HOST_SAMPLES_H

#include <stdint.h>

#include "gten_host.h"
#include "gten_host_fsm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* most samples of one prompt */
#define GTEN_HOST_SAMPLES_MAX 64

/*
 * gten_host_batch_serve_fsm's argument list plus n_samples [n_prompts] (NULL: n_samples_all for every prompt), each in
 * [1, GTEN_HOST_SAMPLES_MAX].  prompts [n_prompts][max_prompt] and n_prompt [n_prompts] speak of the PROMPTS; every other list
 * -- max_new_each, top_k, temp, table, min_new, n_top, top_p, min_p, the lists of pen, fsm_start -- and every output -- out,
 * n_total, logprob_out, top_id_out, top_logprob_out, ended_by -- has one entry (or row) per ITEM of the expanded queue, in
 * expanded order, sized and laid out as gten_host_batch_serve_fsm would for that queue.  0; -1: bad arguments; otherwise the
 * code of the decoder's refusal.
 */
int gten_host_batch_serve_samples(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int n_prompts, int max_prompt, int max_tokens,
                                  int eos, int slice, int max_new, const int32_t* max_new_each, int32_t* out, int32_t* n_total, double* stats, int n_stats,
                                  const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed, const int32_t* table,
                                  const int32_t* min_new, const int32_t* n_top, int n_top_max, float* logprob_out, int32_t* top_id_out,
                                  float* top_logprob_out, const float* top_p, const float* min_p, float top_p_all, float min_p_all,
                                  const gten_host_penalties* pen, const int32_t* fsm_start, int32_t* ended_by, const int32_t* n_samples, int n_samples_all);

/* What the batch's queues saved so far (counted since the batch was made): the items that were copies of another item's prompt
 * pass, the prompt rows not computed for them (behind a registered prefix: the rows the copy would have cost, the prefix's not
 * counted), the groups whose members read from a group record and the marked groups that got none; and the records in use NOW
 * (0 outside a queue).  Any out pointer may be NULL. */
int gten_host_batch_samples_info(gten_host_batch* b, unsigned long long* copies, unsigned long long* rows_saved, unsigned long long* groups_recorded,
                                 unsigned long long* groups_unrecorded, int* records_now);

/* The group records a queue may hold at a time: 0: never take one -- the prompt passes are saved, every member decodes on its
 * own copy; up to GTEN_GROUPS_MAX of include/gten_hip_groups.h (larger values are clamped to it); -1: the library's default,
 * which is GTEN_HOST_GROUPS_CAP_DEFAULT = 0: as measured the records shorten the shared step by 1 % and leave
 * the queue's new tok/s inside the spread of the runs without them. */
#define GTEN_HOST_GROUPS_CAP_DEFAULT 0
int gten_host_batch_set_groups_cap(gten_host_batch* b, int cap);

/* For callers that drive the steps themselves: the group records of the batch's shared decoder (include/gten_hip_groups.h).
 * group_decode_set: record g becomes a snapshot of rows [0, rows) of sequence seq's own caches (seq < 0: released) --
 * gten_hip_decoder_group_set's return code; the caller has waited for whatever wrote those rows.  group_decode_share:
 * gten_hip_decoder_group_share(seq, g, rows), 0 or the refusal's code.  groups_decode_info: gten_hip_decoder_groups_info. */
int gten_host_batch_group_decode_set(gten_host_batch* b, int g, int seq, int rows);
int gten_host_batch_group_decode_share(gten_host_batch* b, int seq, int g, int rows);
int gten_host_batch_groups_decode_info(gten_host_batch* b, int seq, int g, int* group_out, int* chunks_out, int* rows, unsigned long long* imports,
                                       int* sharers);

/* Device-free: the order of a prompt's n samples for best-of-n; order [n] receives the sample indices, best first.  The rule:
 * descending MEAN log-prob per new id, logprob_sum[i] / n_new[i] in double; ties go to the lower sample; a sample without new
 * ids comes last (several of them: by index).  logprob_sum[i] is the sum of sample i's f32 records, formed in double and added
 * in position order.  _rank_records forms these sums itself: records [n][row_len] are the samples' logprob_out rows and
 * n_prompt the prompt's length, so sample i's new ids sit at positions [n_prompt, n_prompt + n_new[i]).  0; -1: bad arguments. */
int gten_host_samples_rank(const double* logprob_sum, const int32_t* n_new, int n, int32_t* order);
int gten_host_samples_rank_records(const float* records, int row_len, int n_prompt, const int32_t* n_new, int n, int32_t* order);

#ifdef __cplusplus
}
#endif

#endif
