// capi_sample.cpp -- flat C exports of sampled generation (include/gten_host_sample.h).  Kept apart from capi.cpp: nothing
// capi.cpp instantiates refers to the sampler's device entry points (include/gten_hip_sample.h).
#include "../../include/gten_host_sample.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "capi_handles.h"

using namespace gten;

namespace {

bool request_ok(int top_k, float temp)
{
    return top_k >= 0 && (top_k == 0 || (std::isfinite(temp) && temp > 0.f));
}

// gten_host_batch_serve2's packing around a serve call: the queue in, the rows and the stats list out
template <class Serve>
int serve_common(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int n_prompts, int max_prompt, int max_tokens, int eos,
                 int slice, int max_new, const int32_t* max_new_each, int32_t* out, int32_t* n_total, double* stats, int n_stats, Serve serve)
{
    (void)eos; (void)max_new; (void)max_new_each;
    if (n_prompts <= 0 || max_tokens <= 0 || slice <= 0) return -1;
    std::vector<std::vector<int32_t>> ps((size_t)n_prompts), res;
    for (int j = 0; j < n_prompts; j++) {
        if (n_prompt[j] <= 0 || n_prompt[j] > max_prompt || n_prompt[j] > b->cfg.max_ctx) return -1;
        ps[(size_t)j].assign(prompts + (size_t)j * max_prompt, prompts + (size_t)j * max_prompt + n_prompt[j]);
    }
    const TinyLlamaBatch::ServeStats st = serve(ps, &res);
    for (int j = 0; j < n_prompts; j++) {
        const int take = std::min((int)res[(size_t)j].size(), std::max(max_tokens, n_prompt[j]));
        std::memcpy(out + (size_t)j * std::max(max_tokens, max_prompt), res[(size_t)j].data(), (size_t)take * sizeof(int32_t));
        n_total[j] = take;
    }
    const double all[] = {(double)st.prompt_tokens, (double)st.new_tokens, (double)st.steps, (double)st.admissions, st.prefill_s, st.decode_s,
                          (double)st.lane_steps, (double)st.lane_rows, (double)st.moved};
    const int have = (int)(sizeof(all) / sizeof(all[0]));
    for (int i = 0; i < n_stats; i++) stats[i] = i < have ? all[i] : 0.0;
    return 0;
}

} // namespace

extern "C" {

int gten_host_model_generate_topk(gten_host_model* m, int32_t* tokens, int n_prompt, int max_tokens, int eos, int top_k, float temp,
                                  uint64_t seed, uint32_t stream)
{
    if (!m || !tokens || n_prompt <= 0 || !request_ok(top_k, temp)) return -1;
    std::vector<int32_t> t(tokens, tokens + n_prompt);
    t.reserve((size_t)std::max(max_tokens, n_prompt));
    const int total = sampled_generate(*m->model, t, max_tokens, eos, top_k, temp, seed, stream);
    if (total < 0) return total;
    std::memcpy(tokens, t.data(), (size_t)total * sizeof(int32_t));
    return total;
}

// gten_host_batch_generate's flow: every prompt on its own caches (the operator path), its first id drawn from its logits row
// on the device, then all sequences generate together with the decoder's sampler; the requests are dropped afterwards.
int gten_host_batch_generate_topk(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int max_prompt, int max_tokens, int eos,
                                  int top_k, float temp, uint64_t seed, const uint32_t* stream, int32_t* out, int32_t* n_total)
{
    if (!b || !prompts || !n_prompt || !out || !n_total || max_tokens <= 0 || !request_ok(top_k, temp)) return -1;
    TinyLlamaBatch& batch = *b->batch;
    const int S = batch.n_seq();
    for (int q = 0; q < S; q++) {
        const int P = n_prompt[q];
        if (P <= 0 || P > max_prompt || P >= max_tokens || P >= b->cfg.max_ctx) return -1;
    }
    // every prompt on its own caches, its first id drawn from its logits row on the device
    std::vector<int32_t> first((size_t)S);
    std::vector<uint32_t> streams((size_t)S);
    for (int q = 0; q < S; q++) {
        const int P = n_prompt[q];
        int32_t* row = out + (size_t)q * max_tokens;
        std::memcpy(row, prompts + (size_t)q * max_prompt, (size_t)P * sizeof(int32_t));
        streams[(size_t)q] = stream ? stream[q] : (uint32_t)q;
        first[(size_t)q] = batch.prefill_sampled(q, std::vector<int32_t>(row, row + P), top_k, temp, seed, streams[(size_t)q]);
    }
    std::vector<int> n_first((size_t)S), room((size_t)S);
    int max_new = 0;
    for (int q = 0; q < S; q++) {
        const int P = n_prompt[q];
        int32_t* row = out + (size_t)q * max_tokens;
        row[P] = first[(size_t)q];                                 // (an eos here ends the sequence below)
        n_first[(size_t)q] = P + 1;
        batch.decode_set_tokens(q, row, 0, P + 1);
        if (const int rc = batch.decode_set_sampling(q, top_k, temp, seed, streams[(size_t)q])) return rc;
        room[(size_t)q] = (first[(size_t)q] == eos) ? 0 : max_tokens - (P + 1);
        max_new = std::max(max_new, room[(size_t)q]);
    }
    std::vector<int32_t> gen((size_t)S * (size_t)std::max(max_new, 1));
    std::vector<int> n_out((size_t)S, 0);
    batch.decode_generate(n_first.data(), max_new, eos, gen.data(), n_out.data(), room.data());
    for (int q = 0; q < S; q++)
        if (const int rc = batch.decode_set_sampling(q, 0, 0.f, 0, 0)) return rc;
    for (int q = 0; q < S; q++) {
        int32_t* row = out + (size_t)q * max_tokens;
        const int total = n_first[(size_t)q];
        if (row[total - 1] == eos) { n_total[q] = total - 1; continue; }
        const int take = std::min(n_out[(size_t)q], max_tokens - total);
        std::memcpy(row + total, gen.data() + (size_t)q * max_new, (size_t)take * sizeof(int32_t));
        n_total[q] = total + take;
    }
    return 0;
}

int gten_host_batch_serve_topk(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int n_prompts, int max_prompt,
                               int max_tokens, int eos, int slice, int max_new, const int32_t* max_new_each, int32_t* out, int32_t* n_total,
                               double* stats, int n_stats, const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed)
{
    if (!b || !prompts || !n_prompt || !out || !n_total || n_prompts < 0 || max_prompt <= 0 || n_stats < 0 || (n_stats > 0 && !stats)) return -1;
    for (int j = 0; j < n_prompts; j++)
        if (!request_ok(top_k ? top_k[j] : top_k_all, temp ? temp[j] : temp_all)) return -1;
    TinyLlamaBatch::SampledServe pick{top_k, temp, top_k_all, temp_all, seed};
    return serve_common(b, prompts, n_prompt, n_prompts, max_prompt, max_tokens, eos, slice, max_new, max_new_each, out, n_total, stats, n_stats,
                        [&](const std::vector<std::vector<int32_t>>& ps, std::vector<std::vector<int32_t>>* got) {
                            return b->batch->serve_with(ps, max_tokens, eos, slice, got, max_new, max_new_each, pick);
                        });
}

} // extern "C"
