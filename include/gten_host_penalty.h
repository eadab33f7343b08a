/*
 * gten_host_penalty.h -- repetition, frequency and presence penalties at the model level (libgten_host.so, host/capi_penalty.cpp),
 * beside include/gten_host_nucleus.h.  The rule is the device's (include/gten_hip_penalty.h): the logit of an id the
 * sequence already holds c times becomes (x > 0 ? x / rep : x * rep) - (c * freq + pres), each operation rounded to f32, before the
 * bias table, the cut and the draw; (rep, freq, pres) = (1, 0, 0) is "no penalty" and gives the ids of the calls without one.  A
 * penalty acts on a greedy request (top_k 0) too.  The ids counted are the last last_n positions before the new id (0: all of them),
 * the prompt's among them (count_prompt != 0) or only generated ones.  Each generation call carries the full request: top-k, table,
 * n_top, the cut and the penalty; records and their outputs as in include/gten_host_nucleus.h.  The first new id is drawn by
 * gten_hip_sample_rows_pen from the prompt's logits row and the prompt's window.  Host pointers throughout; 0 / a count on success,
 * < 0 on bad arguments (rep outside [1/8, 8], |freq| or |pres| > 100, last_n < 0, NaN, ...) or the device library's refusal
 * (gten_hip_last_error).
 */
#ifndef GTEN_HOST_PENALTY_H
#define GTEN_HOST_PENALTY_H

#include <stdint.h>

#include "gten_host_nucleus.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The penalties of a call's items (sequences of a batch, prompts of a queue; a model has one item): each list is [items] or NULL,
 * and NULL means the _all value for everybody.  A zeroed struct is NOT "no penalty" (rep 0 is refused): start from
 * {NULL, NULL, NULL, NULL, NULL, 1, 0, 0, 0, 1}. */
typedef struct gten_host_penalties {
    const float *rep, *freq, *pres;
    const int32_t *last_n, *count_prompt;
    float rep_all, freq_all, pres_all;
    int32_t last_n_all, count_prompt_all;
} gten_host_penalties;

/* For callers that drive the steps themselves: the penalty of the model's decoder / of sequence seq of the batch's shared decoder
 * ((1, 0, 0) clears it; the window is positions [max(start, last_n > 0 ? n - last_n : 0), n) of the decoder's own ids), and every
 * sequence's penalty read back: rep_out / freq_out / pres_out / start_out / last_n_out [n_seq] (1 entry for a model; each may be
 * NULL).  The info calls return 1 when a sequence of the decoder has ever set a penalty, else 0. */
int gten_host_model_set_penalty(gten_host_model* m, float rep, float freq, float pres, int start, int last_n);
int gten_host_batch_set_penalty(gten_host_batch* b, int seq, float rep, float freq, float pres, int start, int last_n);
int gten_host_model_penalty_info(gten_host_model* m, float* rep_out, float* freq_out, float* pres_out, int32_t* start_out, int32_t* last_n_out);
int gten_host_batch_penalty_info(gten_host_batch* b, float* rep_out, float* freq_out, float* pres_out, int32_t* start_out, int32_t* last_n_out);

/* gten_host_model_generate_nucleus under the penalty pen (its _all values; NULL: none).  The request is dropped afterwards. */
int gten_host_model_generate_penalized(gten_host_model* m, int32_t* tokens, int n_prompt, int max_tokens, int eos, int top_k, float temp, uint64_t seed,
                                       uint32_t stream, int table, int min_new, int n_top, float top_p, float min_p, float* logprob_out,
                                       int32_t* top_id_out, float* top_logprob_out, const gten_host_penalties* pen);

/* gten_host_batch_generate_nucleus with a penalty per sequence.  Every request is dropped afterwards, also when a call is refused. */
int gten_host_batch_generate_penalized(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int max_prompt, int max_tokens, int eos,
                                       const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed, const uint32_t* stream,
                                       const int32_t* table, const int32_t* min_new, int32_t* out, int32_t* n_total, const int32_t* n_top, int n_top_max,
                                       float* logprob_out, int32_t* top_id_out, float* top_logprob_out, const float* top_p, const float* min_p,
                                       float top_p_all, float min_p_all, const gten_host_penalties* pen);

/* gten_host_batch_serve_nucleus with a penalty per prompt, set on whichever slot takes the prompt and cleared when the queue is done. */
int gten_host_batch_serve_penalized(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int n_prompts, int max_prompt, int max_tokens,
                                    int eos, int slice, int max_new, const int32_t* max_new_each, int32_t* out, int32_t* n_total, double* stats,
                                    int n_stats, const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed,
                                    const int32_t* table, const int32_t* min_new, const int32_t* n_top, int n_top_max, float* logprob_out,
                                    int32_t* top_id_out, float* top_logprob_out, const float* top_p, const float* min_p, float top_p_all,
                                    float min_p_all, const gten_host_penalties* pen);

#ifdef __cplusplus
}
#endif
#endif
