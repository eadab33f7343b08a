// capi_bias.cpp -- flat C exports of constrained generation (include/gten_host_bias.h): the bias tables and requests of a decoder, and
// host/generate.h's flows with the sampler's and the tables' stages.
#include "../../include/gten_host_bias.h"

#include "capi_handles.h"

using namespace gten;

extern "C" {

int gten_host_model_set_bias_table(gten_host_model* m, int table, const int32_t* ids, const float* values, int n, float fill)
{
    if (!m) return -1;
    return gten_hip_decoder_set_bias_table(m->model->decoder_handle(), table, ids, values, n, fill);
}

int gten_host_batch_set_bias_table(gten_host_batch* b, int table, const int32_t* ids, const float* values, int n, float fill)
{
    if (!b) return -1;
    return gten_hip_decoder_set_bias_table(b->batch->decoder_handle(), table, ids, values, n, fill);
}

int gten_host_batch_set_sampling(gten_host_batch* b, int seq, int top_k, float temp, uint64_t seed, uint32_t stream)
{
    if (!b || !request_ok(top_k, temp)) return -1;
    return gten_hip_decoder_set_sampling(b->batch->decoder_handle(), seq, top_k, temp, seed, stream);
}

int gten_host_batch_set_seq_bias(gten_host_batch* b, int seq, int table, int until)
{
    if (!b) return -1;
    return gten_hip_decoder_set_seq_bias(b->batch->decoder_handle(), seq, table, until);
}

int gten_host_model_set_seq_bias(gten_host_model* m, int table, int until)
{
    if (!m) return -1;
    return gten_hip_decoder_set_seq_bias(m->model->decoder_handle(), 0, table, until);
}

int gten_host_model_set_sampling(gten_host_model* m, int top_k, float temp, uint64_t seed, uint32_t stream)
{
    if (!m || !request_ok(top_k, temp)) return -1;
    return gten_hip_decoder_set_sampling(m->model->decoder_handle(), 0, top_k, temp, seed, stream);
}

int gten_host_model_step_logits(gten_host_model* m, float* logits_out)
{
    if (!m || !logits_out) return -1;
    return gten_hip_decoder_logits_seq(m->model->decoder_handle(), 0, logits_out);
}

int gten_host_batch_bias_info(gten_host_batch* b, int32_t* table_out, int32_t* until_out)
{
    if (!b) return -1;
    int n = 0;
    if (const int rc = gten_hip_decoder_bias_info(b->batch->decoder_handle(), &n, table_out, until_out, -1, nullptr)) return rc;
    return n;
}

int gten_host_model_generate_biased(gten_host_model* m, int32_t* tokens, int n_prompt, int max_tokens, int eos, int top_k, float temp,
                                    uint64_t seed, uint32_t stream, int table, int min_new)
{
    if (!m || !tokens || n_prompt <= 0 || !request_ok(top_k, temp) || !binding_ok(table, min_new)) return -1;
    return generate_in_place<kSampled | kBiased>(*m->model, tokens, n_prompt, max_tokens, eos, Request{top_k, temp, seed, stream, table, min_new});
}

int gten_host_batch_generate_biased(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int max_prompt, int max_tokens, int eos,
                                    const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed, const uint32_t* stream,
                                    const int32_t* table, const int32_t* min_new, int32_t* out, int32_t* n_total)
{
    if (!b || !prompts || !n_prompt || !out || !n_total || max_tokens <= 0) return -1;
    return generate_batch<kSampled | kBiased>(*b->batch, b->cfg.max_ctx, prompts, n_prompt, max_prompt, max_tokens, eos,
                                              Requests::of(top_k, top_k_all, temp, temp_all, seed, stream, table, min_new), out, n_total);
}

int gten_host_batch_serve_biased(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int n_prompts, int max_prompt,
                                 int max_tokens, int eos, int slice, int max_new, const int32_t* max_new_each, int32_t* out, int32_t* n_total,
                                 double* stats, int n_stats, const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed,
                                 const int32_t* table, const int32_t* min_new)
{
    if (!b || !prompts || !n_prompt || !out || !n_total || n_prompts <= 0 || max_prompt <= 0 || n_stats < 0 || (n_stats > 0 && !stats)) return -1;
    return serve_queue<kSampled | kBiased>(*b->batch, b->cfg.max_ctx, prompts, n_prompt, n_prompts, max_prompt, max_tokens, eos, slice, max_new, max_new_each,
                                           out, n_total, stats, n_stats, Requests::of(top_k, top_k_all, temp, temp_all, seed, nullptr, table, min_new));
}

} // extern "C"
