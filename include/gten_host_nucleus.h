/*
 * gten_host_nucleus.h -- top-p (nucleus) and min-p sampling at the model level (libgten_host.so, host/capi_nucleus.cpp), beside
 * include/gten_host_logprobs.h.  The rule is the device's (include/gten_hip_nucleus.h): the kept set is an
 * integer fact about the logits row; (top_p, min_p) = (1, 0) is "no cut" and gives the ids of the calls without one; a greedy
 * request (top_k 0) ignores the cut; nucleus sampling over the whole vocabulary is top_k >= n_vocab.  Each generation call
 * carries the full request: top-k, table, n_top and the cut.  n_top = -1 (n_top NULL, n_top_max 0) asks for no records and the
 * three record outputs may then be NULL; otherwise they are laid out as in include/gten_host_logprobs.h.  The first new id is
 * drawn by gten_hip_sample_rows_cut from the prompt's logits row.  Host pointers throughout; 0 / a count on success, < 0 on bad
 * arguments (top_p outside (0, 1], min_p outside [0, 1], NaN, ...) or the device library's refusal (gten_hip_last_error).
 */
#ifndef GTEN_HOST_NUCLEUS_H
#define GTEN_HOST_NUCLEUS_H

#include <stdint.h>

#include "gten_host_logprobs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* For callers that drive the steps themselves: the cut of the model's decoder / of sequence seq of the batch's shared decoder
 * ((1, 0) clears it), and every sequence's cut read back: top_p_out / min_p_out / t_out [n_seq] (1 entry for a model; each may be
 * NULL), t = (float)log((double)min_p).  The info calls return 1 when a sequence of the decoder has ever set a cut, else 0. */
int gten_host_model_set_cut(gten_host_model* m, float top_p, float min_p);
int gten_host_batch_set_cut(gten_host_batch* b, int seq, float top_p, float min_p);
int gten_host_model_cut_info(gten_host_model* m, float* top_p_out, float* min_p_out, float* t_out);
int gten_host_batch_cut_info(gten_host_batch* b, float* top_p_out, float* min_p_out, float* t_out);

/* gten_host_model_generate_lp under the cut (top_p, min_p).  The request is dropped afterwards. */
int gten_host_model_generate_nucleus(gten_host_model* m, int32_t* tokens, int n_prompt, int max_tokens, int eos, int top_k, float temp, uint64_t seed,
                                     uint32_t stream, int table, int min_new, int n_top, float top_p, float min_p, float* logprob_out,
                                     int32_t* top_id_out, float* top_logprob_out);

/* gten_host_batch_generate_lp with a cut per sequence: top_p / min_p [n_seq], or NULL and top_p_all / min_p_all for everybody.
 * Every request is dropped afterwards, also when a call is refused. */
int gten_host_batch_generate_nucleus(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int max_prompt, int max_tokens, int eos,
                                     const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed, const uint32_t* stream,
                                     const int32_t* table, const int32_t* min_new, int32_t* out, int32_t* n_total, const int32_t* n_top, int n_top_max,
                                     float* logprob_out, int32_t* top_id_out, float* top_logprob_out, const float* top_p, const float* min_p,
                                     float top_p_all, float min_p_all);

/* gten_host_batch_serve_lp with a cut per prompt, set on whichever slot takes the prompt and cleared when the queue is done. */
int gten_host_batch_serve_nucleus(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int n_prompts, int max_prompt, int max_tokens,
                                  int eos, int slice, int max_new, const int32_t* max_new_each, int32_t* out, int32_t* n_total, double* stats,
                                  int n_stats, const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed,
                                  const int32_t* table, const int32_t* min_new, const int32_t* n_top, int n_top_max, float* logprob_out,
                                  int32_t* top_id_out, float* top_logprob_out, const float* top_p, const float* min_p, float top_p_all,
                                  float min_p_all);

#ifdef __cplusplus
}
#endif
#endif
