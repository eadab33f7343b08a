// capi_mirostat.cpp -- flat C exports of include/gten_host_mirostat.h: a sequence's Mirostat binding on a model's or a batch's decoder
// (include/gten_hip_mirostat.h) and generation under Mirostat (host/generate.h's flows with all seven stages -- the only
// instantiation of kMirostat in the library).  The one translation unit of the host library that names the device's Mirostat calls: the
// stub link tests of the other capi files keep linking the smaller masks without them.
#include "../../include/gten_host_mirostat.h"

#include <algorithm>
#include <cstdio>

#include "../../include/gten_hip_mirostat.h"
#include "capi_handles.h"

using namespace gten;

namespace {

constexpr unsigned kSeven = kSampled | kBiased | kLogprobs | kNucleus | kPenalty | kFsm | kMirostat;
const gten_host_penalties kNone = {nullptr, nullptr, nullptr, nullptr, nullptr, 1.f, 0.f, 0.f, 0, 1};

bool records_ok(bool asking, int n_top_max, const float* lp, const int32_t* ids, const float* lps)
{
    if (n_top_max < 0 || n_top_max > GTEN_HIP_LOGPROBS_TOP) return false;
    if (asking && (!lp || (n_top_max > 0 && (!ids || !lps)))) return false;
    return true;
}

Requests with(const Requests& r, const gten_host_penalties* pen, const int32_t* fsm_start, const float* tau, const float* eta, float tau_all, float eta_all)
{
    const gten_host_penalties& p = pen ? *pen : kNone;
    return r.penalised(p.rep, p.rep_all, p.freq, p.freq_all, p.pres, p.pres_all, p.last_n, p.last_n_all, p.count_prompt, p.count_prompt_all)
        .bound_to(fsm_start).with_mirostat(tau, tau_all, eta, eta_all);
}

// a call that carries both a cut and Mirostat on one item is refused by name, before any work
int refuse_pair(const Requests& reqs, int n, const char* who)
{
    for (int j = 0; j < n; j++) {
        const Request r = reqs[j];
        if (r.mirostat() && r.cuts()) {
            std::fprintf(stderr, "%s: item %d asks for a cut (top_p %g, min_p %g) and for mirostat (tau %g): they do not compose\n", who, j, (double)r.top_p,
                         (double)r.min_p, (double)r.miro_tau);
            return -1;
        }
    }
    return 0;
}

int info(gten_hip_decoder* dec, int32_t* tau_q, int32_t* eta_q, int32_t* pos)
{
    int on = 0;
    if (gten_hip_decoder_mirostat_info(dec, tau_q, eta_q, pos, &on, 0, 0, 0, nullptr)) return -1;
    return on;
}

} // namespace

extern "C" {

int gten_host_model_set_mirostat(gten_host_model* m, float tau, float eta, int32_t mu_q16, int pos)
{
    if (!m) return -1;
    return gten_hip_decoder_set_seq_mirostat(m->model->decoder_handle(), 0, tau, eta, mu_q16, pos);
}

int gten_host_batch_set_mirostat(gten_host_batch* b, int seq, float tau, float eta, int32_t mu_q16, int pos)
{
    if (!b) return -1;
    return gten_hip_decoder_set_seq_mirostat(b->batch->decoder_handle(), seq, tau, eta, mu_q16, pos);
}

int gten_host_model_mirostat_info(gten_host_model* m, int32_t* tau_q_out, int32_t* eta_q_out, int32_t* pos_out)
{
    if (!m) return -1;
    return info(m->model->decoder_handle(), tau_q_out, eta_q_out, pos_out);
}

int gten_host_batch_mirostat_info(gten_host_batch* b, int32_t* tau_q_out, int32_t* eta_q_out, int32_t* pos_out)
{
    if (!b) return -1;
    return info(b->batch->decoder_handle(), tau_q_out, eta_q_out, pos_out);
}

int gten_host_model_mirostat_mus(gten_host_model* m, int from, int count, int32_t* mus_out)
{
    if (!m) return -1;
    return gten_hip_decoder_slot_mus(m->model->decoder_handle(), 0, from, count, mus_out);
}

int gten_host_batch_mirostat_mus(gten_host_batch* b, int seq, int from, int count, int32_t* mus_out)
{
    if (!b) return -1;
    return gten_hip_decoder_slot_mus(b->batch->decoder_handle(), seq, from, count, mus_out);
}

int gten_host_model_generate_mirostat(gten_host_model* m, int32_t* tokens, int n_prompt, int max_tokens, int eos, int top_k, float temp, uint64_t seed,
                                      uint32_t stream, int table, int min_new, int n_top, float top_p, float min_p, float* logprob_out,
                                      int32_t* top_id_out, float* top_logprob_out, const gten_host_penalties* pen, int fsm_start, int32_t* ended_by,
                                      float miro_tau, float miro_eta)
{
    if (!m || !tokens || n_prompt <= 0 || max_tokens <= 0 || !request_ok(top_k, temp) || !binding_ok(table, min_new) || !cut_ok(top_p, min_p)) return -1;
    if (n_top < -1 || !records_ok(n_top >= 0, std::max(n_top, 0), logprob_out, top_id_out, top_logprob_out)) return -1;
    const gten_host_penalties& p = pen ? *pen : kNone;
    if (!penalty_ok(p.rep_all, p.freq_all, p.pres_all, p.last_n_all) || !fsm_ok(fsm_start, table)) return -1;
    const RecordRows rows = n_top >= 0 ? RecordRows{logprob_out, top_id_out, top_logprob_out, n_top} : RecordRows{};
    Request r{top_k, temp, seed, stream, table, min_new, n_top, top_p, min_p, p.rep_all, p.freq_all, p.pres_all, p.last_n_all, p.count_prompt_all != 0,
              fsm_start};
    r.miro_tau = miro_tau; r.miro_eta = miro_eta;
    if (r.mirostat() && r.cuts()) {
        std::fprintf(stderr, "model_generate_mirostat: a cut (top_p %g, min_p %g) and mirostat (tau %g) do not compose\n", (double)top_p, (double)min_p,
                     (double)miro_tau);
        return -1;
    }
    if (!mirostat_ok(miro_tau, miro_eta, top_k, top_p, min_p)) return -1;
    int ended = kEndedByLength;
    const int total = generate_in_place<kSeven>(*m->model, tokens, n_prompt, max_tokens, eos, r, rows, &ended, m->cfg.max_ctx);
    if (ended_by) *ended_by = ended;
    return total;
}

int gten_host_batch_generate_mirostat(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int max_prompt, int max_tokens, int eos,
                                      const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed, const uint32_t* stream,
                                      const int32_t* table, const int32_t* min_new, int32_t* out, int32_t* n_total, const int32_t* n_top, int n_top_max,
                                      float* logprob_out, int32_t* top_id_out, float* top_logprob_out, const float* top_p, const float* min_p,
                                      float top_p_all, float min_p_all, const gten_host_penalties* pen, const int32_t* fsm_start, int32_t* ended_by,
                                      const float* miro_tau, const float* miro_eta, float miro_tau_all, float miro_eta_all)
{
    if (!b || !prompts || !n_prompt || !out || !n_total || max_tokens <= 0) return -1;
    if (!records_ok(n_top != nullptr, n_top_max, logprob_out, top_id_out, top_logprob_out)) return -1;
    const RecordRows rows = n_top ? RecordRows{logprob_out, top_id_out, top_logprob_out, n_top_max} : RecordRows{};
    const Requests reqs = with(Requests::of(top_k, top_k_all, temp, temp_all, seed, stream, table, min_new, n_top, top_p, top_p_all, min_p, min_p_all), pen,
                               fsm_start, miro_tau, miro_eta, miro_tau_all, miro_eta_all);
    if (refuse_pair(reqs, b->batch->n_seq(), "batch_generate_mirostat")) return -1;
    return generate_batch<kSeven>(*b->batch, b->cfg.max_ctx, prompts, n_prompt, max_prompt, max_tokens, eos, reqs, out, n_total, rows, ended_by);
}

int gten_host_batch_serve_mirostat(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int n_prompts, int max_prompt, int max_tokens,
                                   int eos, int slice, int max_new, const int32_t* max_new_each, int32_t* out, int32_t* n_total, double* stats,
                                   int n_stats, const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed,
                                   const int32_t* table, const int32_t* min_new, const int32_t* n_top, int n_top_max, float* logprob_out,
                                   int32_t* top_id_out, float* top_logprob_out, const float* top_p, const float* min_p, float top_p_all, float min_p_all,
                                   const gten_host_penalties* pen, const int32_t* fsm_start, int32_t* ended_by, const float* miro_tau,
                                   const float* miro_eta, float miro_tau_all, float miro_eta_all)
{
    if (!b || !prompts || !n_prompt || !out || !n_total || n_prompts <= 0 || max_prompt <= 0 || n_stats < 0 || (n_stats > 0 && !stats)) return -1;
    if (max_tokens <= 0 || slice <= 0) return -1;
    if (!records_ok(n_top != nullptr, n_top_max, logprob_out, top_id_out, top_logprob_out)) return -1;
    const RecordRows rows = n_top ? RecordRows{logprob_out, top_id_out, top_logprob_out, n_top_max} : RecordRows{};
    const Requests reqs = with(Requests::of(top_k, top_k_all, temp, temp_all, seed, nullptr, table, min_new, n_top, top_p, top_p_all, min_p, min_p_all), pen,
                               fsm_start, miro_tau, miro_eta, miro_tau_all, miro_eta_all);
    if (refuse_pair(reqs, n_prompts, "batch_serve_mirostat")) return -1;
    return serve_queue<kSeven>(*b->batch, b->cfg.max_ctx, prompts, n_prompt, n_prompts, max_prompt, max_tokens, eos, slice, max_new, max_new_each, out,
                               n_total, stats, n_stats, reqs, rows, ended_by);
}

} // extern "C"
