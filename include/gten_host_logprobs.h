/*
 * gten_host_logprobs.h -- the log-prob of every generated id and its top-N alternatives at the model level (libgten_host.so,
 * host/capi_logprobs.cpp), beside include/gten_host_bias.h.  The rule is the device's (include/gten_hip_logprobs.h,
 * DESIGN.md §3.11): the numbers come from the step's raw logits row -- no table, temperature 1, the whole vocabulary -- and
 * asking changes no id.  n_top in [0, GTEN_HIP_LOGPROBS_TOP] asks (0: the committed id's log-prob only), -1 does not.
 * The generation calls take the arguments of the _biased ones plus n_top and three outputs aligned with the ids: logprob
 * [..][max_tokens], top_id and top_logprob [..][max_tokens][n_top_max]; positions without a record (the prompt, a prompt that
 * did not ask, entries from its own n_top on) hold logprob 0, id -1.  The first new id's record is computed by
 * gten_hip_row_top_logprobs from the prompt's logits row, the same row the id is drawn from.  Host pointers throughout;
 * 0 / a count on success, < 0 on bad arguments or the device library's refusal (gten_hip_last_error says why).
 */
#ifndef GTEN_HOST_LOGPROBS_H
#define GTEN_HOST_LOGPROBS_H

#include <stdint.h>

#include "gten_host_bias.h"

#ifdef __cplusplus
extern "C" {
#endif

/* For callers that drive the steps themselves (gten_host_model_decode_step, gten_host_batch_decode_step): the request of the
 * model's decoder / of sequence seq of the batch's shared decoder, and the records of positions [n_from, n_from + count) read
 * back (logprob_out [count], top_id_out / top_logprob_out [count][n_top]; waits for the queued steps). */
int gten_host_model_set_logprobs(gten_host_model* m, int n_top);
int gten_host_batch_set_logprobs(gten_host_batch* b, int seq, int n_top);
int gten_host_model_logprobs(gten_host_model* m, int n_from, int count, int n_top, float* logprob_out, int32_t* top_id_out, float* top_logprob_out);
int gten_host_batch_logprobs(gten_host_batch* b, int seq, int n_from, int count, int n_top, float* logprob_out, int32_t* top_id_out,
                             float* top_logprob_out);

/* gten_host_model_generate_biased with records: logprob_out [max_tokens], top_id_out / top_logprob_out [max_tokens][n_top]
 * (n_top >= 0).  The request is dropped afterwards. */
int gten_host_model_generate_lp(gten_host_model* m, int32_t* tokens, int n_prompt, int max_tokens, int eos, int top_k, float temp, uint64_t seed,
                                uint32_t stream, int table, int min_new, int n_top, float* logprob_out, int32_t* top_id_out, float* top_logprob_out);

/* gten_host_batch_generate_biased with n_top[q] per sequence (NULL: nobody asks); the outputs are [n_seq][max_tokens] and
 * [n_seq][max_tokens][n_top_max], n_top_max >= every n_top[q].  Every request is dropped afterwards. */
int gten_host_batch_generate_lp(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int max_prompt, int max_tokens, int eos,
                                const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed, const uint32_t* stream,
                                const int32_t* table, const int32_t* min_new, int32_t* out, int32_t* n_total, const int32_t* n_top, int n_top_max,
                                float* logprob_out, int32_t* top_id_out, float* top_logprob_out);

/* gten_host_batch_serve_biased with n_top[j] per prompt (NULL: nobody asks).  A prompt's row of out and of the three outputs
 * is max(max_tokens, max_prompt) positions long.  A slot's records are read when its prompt ends (or moves to another slot),
 * before the slot is started again; every slot's request is cleared when the queue is done. */
int gten_host_batch_serve_lp(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int n_prompts, int max_prompt, int max_tokens,
                             int eos, int slice, int max_new, const int32_t* max_new_each, int32_t* out, int32_t* n_total, double* stats, int n_stats,
                             const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed, const int32_t* table,
                             const int32_t* min_new, const int32_t* n_top, int n_top_max, float* logprob_out, int32_t* top_id_out,
                             float* top_logprob_out);

/* gten_host_model_score plus the top-N of every scored row: top_id_out / top_logprob_out [n - start_pos][n_top].  The operator
 * runs beside gten_hip_row_logprobs in the same chunks; logprob_out is gten_host_model_score's. */
int gten_host_model_score_top(gten_host_model* m, const int32_t* tokens, int n, int start_pos, const int32_t* targets, int n_top,
                              float* logprob_out, int32_t* rank_out, int32_t* top_id_out, float* top_logprob_out);

#ifdef __cplusplus
}
#endif
#endif
