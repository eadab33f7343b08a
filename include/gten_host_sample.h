/*
 * gten_host_sample.h -- top-k sampling with a temperature at the model level (libgten_host.so, host/capi_sample.cpp),
 * beside include/gten_host.h.  The draw is the device sampler's contract (include/gten_hip_sample.h):
 * the id at position p depends only on the logits that produce it and on (seed, stream).  top_k == 0 gives the greedy
 * entry points' ids; top_k >= 1 wants a finite temp > 0.  Host pointers throughout; 0 / a count on success, < 0 on bad
 * arguments.
 */
#ifndef GTEN_HOST_SAMPLE_H
#define GTEN_HOST_SAMPLE_H

#include <stdint.h>

#include "gten_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gten_host_model_generate with every new id sampled (the prompt's first one from its logits on the device, the others by
 * the decoder's sampler): same arguments and return value, plus the request and the stream of this sequence. */
int gten_host_model_generate_topk(gten_host_model* m, int32_t* tokens, int n_prompt, int max_tokens, int eos, int top_k, float temp,
                                  uint64_t seed, uint32_t stream);
/* gten_host_batch_generate with every new id sampled; sequence q draws with stream[q] (stream NULL: q). */
int gten_host_batch_generate_topk(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int max_prompt, int max_tokens, int eos,
                                  int top_k, float temp, uint64_t seed, const uint32_t* stream, int32_t* out, int32_t* n_total);

/* gten_host_batch_serve2 with every new id sampled: prompt j draws with top_k[j] / temp[j] (NULL: top_k_all / temp_all for
 * every prompt; top_k 0 = greedy, so greedy and sampled prompts share one queue), the one seed, and stream j -- its index in
 * the queue.  Its ids then do not depend on the slot it lands on, the number of slots or the admission schedule. */
int gten_host_batch_serve_topk(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int n_prompts, int max_prompt,
                               int max_tokens, int eos, int slice, int max_new, const int32_t* max_new_each, int32_t* out, int32_t* n_total,
                               double* stats, int n_stats, const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed);

#ifdef __cplusplus
}
#endif
#endif
