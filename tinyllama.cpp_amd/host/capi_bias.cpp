// capi_bias.cpp -- flat C exports of constrained generation (include/gten_host_bias.h).  Kept apart from capi.cpp and
// capi_sample.cpp: this is the only translation unit that instantiates code referring to the bias tables' device entry points
// (include/gten_hip_bias.h).
#include "../../include/gten_host_bias.h"

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
bool binding_ok(int table, int min_new)
{
    return table >= -1 && table < GTEN_HIP_BIAS_TABLES && min_new >= 0;
}

} // namespace

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
    return b->batch->decode_set_sampling(seq, top_k, temp, seed, stream);
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
    return m->model->decode_set_sampling(top_k, temp, seed, stream);
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
    std::vector<int32_t> t(tokens, tokens + n_prompt);
    t.reserve((size_t)std::max(max_tokens, n_prompt));
    const int total = biased_generate(*m->model, t, max_tokens, eos, top_k, temp, seed, stream, table, min_new);
    if (total < 0) return total;
    std::memcpy(tokens, t.data(), (size_t)total * sizeof(int32_t));
    return total;
}

// gten_host_batch_generate_topk's flow with a request and a binding per sequence
int gten_host_batch_generate_biased(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int max_prompt, int max_tokens, int eos,
                                    const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed, const uint32_t* stream,
                                    const int32_t* table, const int32_t* min_new, int32_t* out, int32_t* n_total)
{
    if (!b || !prompts || !n_prompt || !out || !n_total || max_tokens <= 0) return -1;
    TinyLlamaBatch& batch = *b->batch;
    const int S = batch.n_seq();
    auto k_of = [&](int q) { return top_k ? top_k[q] : top_k_all; };
    auto t_of = [&](int q) { return temp ? temp[q] : temp_all; };
    auto tab_of = [&](int q) { return table ? table[q] : -1; };
    auto until_of = [&](int q) { return (tab_of(q) >= 0 && min_new && min_new[q] > 0) ? n_prompt[q] + min_new[q] : 0; };
    for (int q = 0; q < S; q++) {
        const int P = n_prompt[q];
        if (P <= 0 || P > max_prompt || P >= max_tokens || P >= b->cfg.max_ctx) return -1;
        if (!request_ok(k_of(q), t_of(q)) || !binding_ok(tab_of(q), min_new ? min_new[q] : 0)) return -1;
    }
    gten_hip_decoder* dec = batch.decoder_handle();
    auto reset = [&]() {
        int rc = 0;
        for (int q = 0; q < S; q++) {
            if (const int r = batch.decode_set_sampling(q, 0, 0.f, 0, 0)) rc = r;
            if (const int r = gten_hip_decoder_set_seq_bias(dec, q, -1, 0)) rc = r;
        }
        return rc;
    };
    // the bindings first: a refusal (a persistent decoder) before any work
    for (int q = 0; q < S; q++)
        if (const int rc = gten_hip_decoder_set_seq_bias(dec, q, tab_of(q), until_of(q))) { reset(); return rc; }
    // every prompt on its own caches, its first id drawn from its logits row on the device under its table
    std::vector<int32_t> first((size_t)S);
    std::vector<uint32_t> streams((size_t)S);
    for (int q = 0; q < S; q++) {
        const int P = n_prompt[q];
        int32_t* row = out + (size_t)q * max_tokens;
        std::memcpy(row, prompts + (size_t)q * max_prompt, (size_t)P * sizeof(int32_t));
        streams[(size_t)q] = stream ? stream[q] : (uint32_t)q;
        const int32_t kk = k_of(q), pos = P;
        const float t = t_of(q);
        const float* brow = nullptr;
        if (tab_of(q) >= 0 && gten_hip_decoder_bias_info(dec, nullptr, nullptr, nullptr, tab_of(q), &brow) != 0) { reset(); return -1; }
        first[(size_t)q] = batch.prefill_picked(q, std::vector<int32_t>(row, row + P), [&](int, const float* lg, int n, int32_t* id) {
            if (brow) GTEN_HIP_OK(gten_hip_sample_rows_biased(lg, 1, n, 0, brow, 0, &kk, &t, seed, &streams[(size_t)q], &pos, id));
            else GTEN_HIP_OK(gten_hip_sample_rows(lg, 1, n, 0, &kk, &t, seed, &streams[(size_t)q], &pos, id));
        });
    }
    std::vector<int> n_first((size_t)S), room((size_t)S);
    int max_new = 0;
    for (int q = 0; q < S; q++) {
        const int P = n_prompt[q];
        int32_t* row = out + (size_t)q * max_tokens;
        row[P] = first[(size_t)q];                                 // (an eos here ends the sequence below)
        n_first[(size_t)q] = P + 1;
        batch.decode_set_tokens(q, row, 0, P + 1);
        if (const int rc = batch.decode_set_sampling(q, k_of(q), t_of(q), seed, streams[(size_t)q])) { reset(); return rc; }
        room[(size_t)q] = (first[(size_t)q] == eos) ? 0 : max_tokens - (P + 1);
        max_new = std::max(max_new, room[(size_t)q]);
    }
    std::vector<int32_t> gen((size_t)S * (size_t)std::max(max_new, 1));
    std::vector<int> n_out((size_t)S, 0);
    batch.decode_generate(n_first.data(), max_new, eos, gen.data(), n_out.data(), room.data());
    if (const int rc = reset()) return rc;
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

int gten_host_batch_serve_biased(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int n_prompts, int max_prompt,
                                 int max_tokens, int eos, int slice, int max_new, const int32_t* max_new_each, int32_t* out, int32_t* n_total,
                                 double* stats, int n_stats, const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed,
                                 const int32_t* table, const int32_t* min_new)
{
    if (!b || !prompts || !n_prompt || !out || !n_total || n_prompts <= 0 || max_prompt <= 0 || n_stats < 0 || (n_stats > 0 && !stats)) return -1;
    if (max_tokens <= 0 || slice <= 0) return -1;
    for (int j = 0; j < n_prompts; j++) {
        if (!request_ok(top_k ? top_k[j] : top_k_all, temp ? temp[j] : temp_all)) return -1;
        if (!binding_ok(table ? table[j] : -1, min_new ? min_new[j] : 0)) return -1;
        if (n_prompt[j] <= 0 || n_prompt[j] > max_prompt || n_prompt[j] > b->cfg.max_ctx) return -1;
    }
    gten_hip_decoder* dec = b->batch->decoder_handle();
    // a decoder that refuses tables says so before the queue starts (slot 0 is unbound again at once)
    if (table) {
        if (const int rc = gten_hip_decoder_set_seq_bias(dec, 0, 0, 0)) return rc;
        if (const int rc = gten_hip_decoder_set_seq_bias(dec, 0, -1, 0)) return rc;
    }
    TinyLlamaBatch::BiasedServe pick{top_k, temp, top_k_all, temp_all, seed, table, min_new, dec};
    std::vector<std::vector<int32_t>> ps((size_t)n_prompts), res;
    for (int j = 0; j < n_prompts; j++)
        ps[(size_t)j].assign(prompts + (size_t)j * max_prompt, prompts + (size_t)j * max_prompt + n_prompt[j]);
    const TinyLlamaBatch::ServeStats st = b->batch->serve_with(ps, max_tokens, eos, slice, &res, max_new, max_new_each, pick);
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

} // extern "C"
