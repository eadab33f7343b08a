// capi_penalty.cpp -- flat C exports of include/gten_host_penalty.h: generation under repetition / frequency / presence penalties
// (host/generate.h's flows with all five stages -- the only instantiation of kPenalty in the library).
#include "../../include/gten_host_penalty.h"

#include <vector>

#include "capi_handles.h"

using namespace gten;

namespace {

constexpr unsigned kAll = kSampled | kBiased | kLogprobs | kNucleus | kPenalty;
const gten_host_penalties kNone = {nullptr, nullptr, nullptr, nullptr, nullptr, 1.f, 0.f, 0.f, 0, 1};

bool records_ok(bool asking, int n_top_max, const float* lp, const int32_t* ids, const float* lps)
{
    if (n_top_max < 0 || n_top_max > GTEN_HIP_LOGPROBS_TOP) return false;
    if (asking && (!lp || (n_top_max > 0 && (!ids || !lps)))) return false;
    return true;
}

Requests with(const Requests& r, const gten_host_penalties* pen)
{
    const gten_host_penalties& p = pen ? *pen : kNone;
    return r.penalised(p.rep, p.rep_all, p.freq, p.freq_all, p.pres, p.pres_all, p.last_n, p.last_n_all, p.count_prompt, p.count_prompt_all);
}

int info(gten_hip_decoder* dec, float* rep, float* freq, float* pres, int32_t* start, int32_t* last_n)
{
    int on = 0;
    if (gten_hip_decoder_penalty_info(dec, rep, freq, pres, start, last_n, &on)) return -1;
    return on;
}

} // namespace

extern "C" {

int gten_host_model_set_penalty(gten_host_model* m, float rep, float freq, float pres, int start, int last_n)
{
    if (!m) return -1;
    return gten_hip_decoder_set_penalty(m->model->decoder_handle(), 0, rep, freq, pres, start, last_n);
}

int gten_host_batch_set_penalty(gten_host_batch* b, int seq, float rep, float freq, float pres, int start, int last_n)
{
    if (!b) return -1;
    return gten_hip_decoder_set_penalty(b->batch->decoder_handle(), seq, rep, freq, pres, start, last_n);
}

int gten_host_model_penalty_info(gten_host_model* m, float* rep_out, float* freq_out, float* pres_out, int32_t* start_out, int32_t* last_n_out)
{
    if (!m) return -1;
    return info(m->model->decoder_handle(), rep_out, freq_out, pres_out, start_out, last_n_out);
}

int gten_host_batch_penalty_info(gten_host_batch* b, float* rep_out, float* freq_out, float* pres_out, int32_t* start_out, int32_t* last_n_out)
{
    if (!b) return -1;
    return info(b->batch->decoder_handle(), rep_out, freq_out, pres_out, start_out, last_n_out);
}

int gten_host_model_generate_penalized(gten_host_model* m, int32_t* tokens, int n_prompt, int max_tokens, int eos, int top_k, float temp, uint64_t seed,
                                       uint32_t stream, int table, int min_new, int n_top, float top_p, float min_p, float* logprob_out,
                                       int32_t* top_id_out, float* top_logprob_out, const gten_host_penalties* pen)
{
    if (!m || !tokens || n_prompt <= 0 || max_tokens <= 0 || !request_ok(top_k, temp) || !binding_ok(table, min_new) || !cut_ok(top_p, min_p)) return -1;
    if (n_top < -1 || !records_ok(n_top >= 0, std::max(n_top, 0), logprob_out, top_id_out, top_logprob_out)) return -1;
    const gten_host_penalties& p = pen ? *pen : kNone;
    if (!penalty_ok(p.rep_all, p.freq_all, p.pres_all, p.last_n_all)) return -1;
    const RecordRows rows = n_top >= 0 ? RecordRows{logprob_out, top_id_out, top_logprob_out, n_top} : RecordRows{};
    const Request r{top_k, temp, seed, stream, table, min_new, n_top, top_p, min_p, p.rep_all, p.freq_all, p.pres_all, p.last_n_all, p.count_prompt_all != 0};
    return generate_in_place<kAll>(*m->model, tokens, n_prompt, max_tokens, eos, r, rows);
}

int gten_host_batch_generate_penalized(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int max_prompt, int max_tokens, int eos,
                                       const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed, const uint32_t* stream,
                                       const int32_t* table, const int32_t* min_new, int32_t* out, int32_t* n_total, const int32_t* n_top, int n_top_max,
                                       float* logprob_out, int32_t* top_id_out, float* top_logprob_out, const float* top_p, const float* min_p,
                                       float top_p_all, float min_p_all, const gten_host_penalties* pen)
{
    if (!b || !prompts || !n_prompt || !out || !n_total || max_tokens <= 0) return -1;
    if (!records_ok(n_top != nullptr, n_top_max, logprob_out, top_id_out, top_logprob_out)) return -1;
    const RecordRows rows = n_top ? RecordRows{logprob_out, top_id_out, top_logprob_out, n_top_max} : RecordRows{};
    return generate_batch<kAll>(*b->batch, b->cfg.max_ctx, prompts, n_prompt, max_prompt, max_tokens, eos,
                                with(Requests::of(top_k, top_k_all, temp, temp_all, seed, stream, table, min_new, n_top, top_p, top_p_all, min_p, min_p_all), pen),
                                out, n_total, rows);
}

int gten_host_batch_serve_penalized(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int n_prompts, int max_prompt, int max_tokens,
                                    int eos, int slice, int max_new, const int32_t* max_new_each, int32_t* out, int32_t* n_total, double* stats,
                                    int n_stats, const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed,
                                    const int32_t* table, const int32_t* min_new, const int32_t* n_top, int n_top_max, float* logprob_out,
                                    int32_t* top_id_out, float* top_logprob_out, const float* top_p, const float* min_p, float top_p_all,
                                    float min_p_all, const gten_host_penalties* pen)
{
    if (!b || !prompts || !n_prompt || !out || !n_total || n_prompts <= 0 || max_prompt <= 0 || n_stats < 0 || (n_stats > 0 && !stats)) return -1;
    if (max_tokens <= 0 || slice <= 0) return -1;
    if (!records_ok(n_top != nullptr, n_top_max, logprob_out, top_id_out, top_logprob_out)) return -1;
    const RecordRows rows = n_top ? RecordRows{logprob_out, top_id_out, top_logprob_out, n_top_max} : RecordRows{};
    return serve_queue<kAll>(*b->batch, b->cfg.max_ctx, prompts, n_prompt, n_prompts, max_prompt, max_tokens, eos, slice, max_new, max_new_each, out, n_total,
                             stats, n_stats,
                             with(Requests::of(top_k, top_k_all, temp, temp_all, seed, nullptr, table, min_new, n_top, top_p, top_p_all, min_p, min_p_all), pen),
                             rows);
}

} // extern "C"
