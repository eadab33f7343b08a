// capi_sample.cpp -- flat C exports of sampled generation (include/gten_host_sample.h): host/generate.h's flows with the sampler's stage.
#include "../../include/gten_host_sample.h"

#include "capi_handles.h"

using namespace gten;

extern "C" {

int gten_host_model_generate_topk(gten_host_model* m, int32_t* tokens, int n_prompt, int max_tokens, int eos, int top_k, float temp,
                                  uint64_t seed, uint32_t stream)
{
    if (!m || !tokens || n_prompt <= 0 || !request_ok(top_k, temp)) return -1;
    return generate_in_place<kSampled>(*m->model, tokens, n_prompt, max_tokens, eos, Request{top_k, temp, seed, stream});
}

int gten_host_batch_generate_topk(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int max_prompt, int max_tokens, int eos,
                                  int top_k, float temp, uint64_t seed, const uint32_t* stream, int32_t* out, int32_t* n_total)
{
    if (!b || !prompts || !n_prompt || !out || !n_total || max_tokens <= 0) return -1;
    return generate_batch<kSampled>(*b->batch, b->cfg.max_ctx, prompts, n_prompt, max_prompt, max_tokens, eos,
                                    Requests::of(nullptr, top_k, nullptr, temp, seed, stream), out, n_total);
}

int gten_host_batch_serve_topk(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int n_prompts, int max_prompt,
                               int max_tokens, int eos, int slice, int max_new, const int32_t* max_new_each, int32_t* out, int32_t* n_total,
                               double* stats, int n_stats, const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed)
{
    if (!b || !prompts || !n_prompt || !out || !n_total || n_prompts < 0 || max_prompt <= 0 || n_stats < 0 || (n_stats > 0 && !stats)) return -1;
    return serve_queue<kSampled>(*b->batch, b->cfg.max_ctx, prompts, n_prompt, n_prompts, max_prompt, max_tokens, eos, slice, max_new, max_new_each, out,
                                 n_total, stats, n_stats, Requests::of(top_k, top_k_all, temp, temp_all, seed));
}

} // extern "C"
