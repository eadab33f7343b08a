/*
 * gten_host_bias.h -- constrained generation at the model level (libgten_host.so, host/capi_bias.cpp), beside
 * include/gten_host_sample.h.  The rule is the device's (include/gten_hip_bias.h): a model or a batch owns
 * GTEN_HIP_BIAS_TABLES bias tables of n_vocab f32 entries; a sequence or a prompt names one (table, -1: none) and a
 * min_new: the table holds for its first min_new new ids (0: for all of them) -- the host turns that into the device's
 * until = n_prompt + min_new.  Every new id obeys it, the first one after the prompt included.  Host pointers throughout;
 * 0 / a count on success, < 0 on bad arguments or the device library's refusal (gten_hip_last_error says why).
 */
#ifndef GTEN_HOST_BIAS_H
#define GTEN_HOST_BIAS_H

#include <stdint.h>

#include "gten_host_sample.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Table `table` := `fill` everywhere, then values[i] at ids[i] (gten_hip_decoder_set_bias_table).  A refused request leaves
 * the table as it was. */
int gten_host_model_set_bias_table(gten_host_model* m, int table, const int32_t* ids, const float* values, int n, float fill);
int gten_host_batch_set_bias_table(gten_host_batch* b, int table, const int32_t* ids, const float* values, int n, float fill);

/* The pieces the generation calls below are made of, for callers that drive the steps themselves (gten_host_batch_decode_step):
 * sequence seq's request and its binding on the batch's shared decoder, and the bindings read back (table_out / until_out:
 * [n_seq] or NULL; returns the number of tables). */
int gten_host_batch_set_sampling(gten_host_batch* b, int seq, int top_k, float temp, uint64_t seed, uint32_t stream);
int gten_host_batch_set_seq_bias(gten_host_batch* b, int seq, int table, int until);
int gten_host_batch_bias_info(gten_host_batch* b, int32_t* table_out, int32_t* until_out);
int gten_host_model_set_seq_bias(gten_host_model* m, int table, int until);
/* The same for a model's single-sequence decoder, and the logits row its last decode step produced (f32 [n_vocab]). */
int gten_host_model_set_sampling(gten_host_model* m, int top_k, float temp, uint64_t seed, uint32_t stream);
int gten_host_model_step_logits(gten_host_model* m, float* logits_out);

/* gten_host_model_generate_topk under a table (top_k 0: greedy over the biased logits).  The binding is dropped afterwards. */
int gten_host_model_generate_biased(gten_host_model* m, int32_t* tokens, int n_prompt, int max_tokens, int eos, int top_k, float temp,
                                    uint64_t seed, uint32_t stream, int table, int min_new);

/* gten_host_batch_generate_topk with a request per sequence: top_k[q], temp[q] (NULL: top_k_all / temp_all), stream[q]
 * (NULL: q), table[q] (NULL: -1), min_new[q] (NULL: 0).  One batch may mix constrained and unconstrained, greedy and sampled
 * sequences.  Every request and binding is dropped afterwards. */
int gten_host_batch_generate_biased(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int max_prompt, int max_tokens, int eos,
                                    const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed, const uint32_t* stream,
                                    const int32_t* table, const int32_t* min_new, int32_t* out, int32_t* n_total);

/* gten_host_batch_serve_topk with a table and a min_new per prompt (either list NULL: none).  Prompt j's ids depend on its
 * logits, its request and its table only; every slot is unbound again afterwards. */
int gten_host_batch_serve_biased(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int n_prompts, int max_prompt,
                                 int max_tokens, int eos, int slice, int max_new, const int32_t* max_new_each, int32_t* out, int32_t* n_total,
                                 double* stats, int n_stats, const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed,
                                 const int32_t* table, const int32_t* min_new);

#ifdef __cplusplus
}
#endif
#endif
