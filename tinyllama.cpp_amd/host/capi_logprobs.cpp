// capi_logprobs.cpp -- flat C exports of include/gten_host_logprobs.h: generation that reports every new id's log-prob and top-N
// alternatives (host/generate.h's flows with all three stages), and scoring with alternatives.
#include "../../include/gten_host_logprobs.h"

#include <algorithm>
#include <cstring>
#include <vector>

#include "capi_handles.h"

using namespace gten;

namespace {

constexpr unsigned kAll = kSampled | kBiased | kLogprobs;

} // namespace

extern "C" {

int gten_host_model_set_logprobs(gten_host_model* m, int n_top)
{
    if (!m) return -1;
    return gten_hip_decoder_set_logprobs(m->model->decoder_handle(), 0, n_top);
}

int gten_host_batch_set_logprobs(gten_host_batch* b, int seq, int n_top)
{
    if (!b) return -1;
    return gten_hip_decoder_set_logprobs(b->batch->decoder_handle(), seq, n_top);
}

int gten_host_model_logprobs(gten_host_model* m, int n_from, int count, int n_top, float* logprob_out, int32_t* top_id_out, float* top_logprob_out)
{
    if (!m) return -1;
    return gten_hip_decoder_logprobs(m->model->decoder_handle(), 0, n_from, count, n_top, logprob_out, top_id_out, top_logprob_out);
}

int gten_host_batch_logprobs(gten_host_batch* b, int seq, int n_from, int count, int n_top, float* logprob_out, int32_t* top_id_out,
                             float* top_logprob_out)
{
    if (!b) return -1;
    return gten_hip_decoder_logprobs(b->batch->decoder_handle(), seq, n_from, count, n_top, logprob_out, top_id_out, top_logprob_out);
}

int gten_host_model_generate_lp(gten_host_model* m, int32_t* tokens, int n_prompt, int max_tokens, int eos, int top_k, float temp, uint64_t seed,
                                uint32_t stream, int table, int min_new, int n_top, float* logprob_out, int32_t* top_id_out, float* top_logprob_out)
{
    if (!m || !tokens || n_prompt <= 0 || max_tokens <= 0 || !request_ok(top_k, temp) || !binding_ok(table, min_new)) return -1;
    if (n_top < 0 || n_top > GTEN_HIP_LOGPROBS_TOP || !logprob_out || (n_top > 0 && (!top_id_out || !top_logprob_out))) return -1;
    return generate_in_place<kAll>(*m->model, tokens, n_prompt, max_tokens, eos, Request{top_k, temp, seed, stream, table, min_new, n_top},
                                   RecordRows{logprob_out, top_id_out, top_logprob_out, n_top});
}

int gten_host_batch_generate_lp(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int max_prompt, int max_tokens, int eos,
                                const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed, const uint32_t* stream,
                                const int32_t* table, const int32_t* min_new, int32_t* out, int32_t* n_total, const int32_t* n_top, int n_top_max,
                                float* logprob_out, int32_t* top_id_out, float* top_logprob_out)
{
    if (!b || !prompts || !n_prompt || !out || !n_total || max_tokens <= 0) return -1;
    if (n_top_max < 0 || n_top_max > GTEN_HIP_LOGPROBS_TOP || !logprob_out || (n_top_max > 0 && (!top_id_out || !top_logprob_out))) return -1;
    return generate_batch<kAll>(*b->batch, b->cfg.max_ctx, prompts, n_prompt, max_prompt, max_tokens, eos,
                                Requests::of(top_k, top_k_all, temp, temp_all, seed, stream, table, min_new, n_top), out, n_total,
                                RecordRows{logprob_out, top_id_out, top_logprob_out, n_top_max});
}

int gten_host_batch_serve_lp(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int n_prompts, int max_prompt, int max_tokens,
                             int eos, int slice, int max_new, const int32_t* max_new_each, int32_t* out, int32_t* n_total, double* stats, int n_stats,
                             const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed, const int32_t* table,
                             const int32_t* min_new, const int32_t* n_top, int n_top_max, float* logprob_out, int32_t* top_id_out,
                             float* top_logprob_out)
{
    if (!b || !prompts || !n_prompt || !out || !n_total || n_prompts <= 0 || max_prompt <= 0 || n_stats < 0 || (n_stats > 0 && !stats)) return -1;
    if (max_tokens <= 0 || slice <= 0) return -1;
    if (n_top_max < 0 || n_top_max > GTEN_HIP_LOGPROBS_TOP || !logprob_out || (n_top_max > 0 && (!top_id_out || !top_logprob_out))) return -1;
    return serve_queue<kAll>(*b->batch, b->cfg.max_ctx, prompts, n_prompt, n_prompts, max_prompt, max_tokens, eos, slice, max_new, max_new_each, out, n_total,
                             stats, n_stats, Requests::of(top_k, top_k_all, temp, temp_all, seed, nullptr, table, min_new, n_top), RecordRows{logprob_out, top_id_out, top_logprob_out, n_top_max});
}

int gten_host_model_score_top(gten_host_model* m, const int32_t* tokens, int n, int start_pos, const int32_t* targets, int n_top,
                              float* logprob_out, int32_t* rank_out, int32_t* top_id_out, float* top_logprob_out)
{
    if (!m || !tokens || n < 1 || n > m->cfg.max_ctx || start_pos < 0 || start_pos >= n || !targets || !logprob_out) return -1;
    if (n_top < 0 || n_top > GTEN_HIP_LOGPROBS_TOP || (n_top > 0 && (!top_id_out || !top_logprob_out))) return -1;
    const int rows = n - start_pos, V = m->cfg.n_vocab;
    for (int i = 0; i < rows; i++)
        if (targets[i] < -1 || targets[i] >= V) return -1;
    // targets | log-probs | ranks | the operator's log-probs (unused: the scorer's are returned) | top ids | top log-probs
    void* io = nullptr;
    const size_t R = (size_t)rows, T = (size_t)std::max(n_top, 1);
    GTEN_HIP_OK(gten_hip_malloc(&io, R * 4 * (4 + 2 * T)));
    int32_t* tdev = (int32_t*)io;
    float* lp = (float*)(tdev + R);
    int32_t* rk = (int32_t*)(lp + R);
    float* lp2 = (float*)(rk + R);
    int32_t* tid = (int32_t*)(lp2 + R);
    float* tlp = (float*)(tid + R * T);
    GTEN_HIP_OK(gten_hip_memcpy_h2d(tdev, targets, R * sizeof(int32_t)));
    Tensor tk(tokens, {n}, kInt32);
    m->model->rows_logits(tk, start_pos, [&](const float* lg, int r0, int cr, long long stride) {
        GTEN_HIP_OK(gten_hip_row_logprobs(lg, cr, V, stride, tdev + r0, lp + r0, rk + r0, nullptr));
        GTEN_HIP_OK(gten_hip_row_top_logprobs(lg, cr, V, stride, tdev + r0, n_top, lp2 + r0, tid + (size_t)r0 * n_top, tlp + (size_t)r0 * n_top));
    });
    GTEN_HIP_OK(gten_hip_memcpy_d2h(logprob_out, lp, R * sizeof(float)));
    if (rank_out) GTEN_HIP_OK(gten_hip_memcpy_d2h(rank_out, rk, R * sizeof(int32_t)));
    if (n_top > 0) {
        GTEN_HIP_OK(gten_hip_memcpy_d2h(top_id_out, tid, R * (size_t)n_top * sizeof(int32_t)));
        GTEN_HIP_OK(gten_hip_memcpy_d2h(top_logprob_out, tlp, R * (size_t)n_top * sizeof(float)));
    }
    GTEN_HIP_OK(gten_hip_free(io));
    return 0;
}

} // extern "C"
