// capi_flows.h -- host/generate.h's three flows at kFull as plain functions, and what every export above kSampled needs to call them.
// host/capi_generate.cpp defines the functions and is the only translation unit of the library that instantiates the kFull flows;
// host/capi_bias.cpp ... host/capi_mirostat.cpp, host/capi_sessions.cpp, host/capi_samples.cpp and host/capi_shift.cpp hold adapters: each
// checks its own arguments, packs a Request / Requests / RecordRows with the helpers below and calls one of the three.  An export
// that cannot pass a stage leaves it at its default, and a stage no request uses costs no decoder call (SlotRequests).
#pragma once

#include "../../include/gten_host_penalty.h"
#include "capi_handles.h"

namespace gten {

// generate_in_place, generate_batch and serve_queue at kFull: their arguments, their return codes
int generate_full(TinyLlama& model, int32_t* tokens, int n_prompt, int max_tokens, int eos, const Request& r, const RecordRows& rows = {},
                  int* ended_by = nullptr, int max_ctx = 0);
int generate_batch_full(TinyLlamaBatch& batch, int max_ctx, const int32_t* prompts, const int32_t* n_prompt, int max_prompt, int max_tokens, int eos,
                        const Requests& reqs, int32_t* out, int32_t* n_total, const RecordRows& rows = {}, int32_t* ended_by = nullptr);
int serve_queue_full(TinyLlamaBatch& batch, int max_ctx, const int32_t* prompts, const int32_t* n_prompt, int n_prompts, int max_prompt, int max_tokens,
                     int eos, int slice, int max_new, const int32_t* max_new_each, int32_t* out, int32_t* n_total, double* stats, int n_stats,
                     const Requests& reqs, const RecordRows& rows = {}, int32_t* ended_by = nullptr, const int32_t* group_of = nullptr,
                     const int32_t* session = nullptr);

// the pointer and count arguments every fixed-batch / every queue export takes
inline bool batch_args_ok(const gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, const int32_t* out, const int32_t* n_total, int max_tokens)
{
    return b && prompts && n_prompt && out && n_total && max_tokens > 0;
}
inline bool serve_args_ok(const gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, const int32_t* out, const int32_t* n_total, int n_prompts,
                          int max_prompt, const double* stats, int n_stats)
{
    return b && prompts && n_prompt && out && n_total && n_prompts > 0 && max_prompt > 0 && n_stats >= 0 && (n_stats == 0 || stats);
}

// n_top_max / the three outputs of a call whose requests ask for at most n_top_max alternatives (nobody asks: none needed) ...
inline bool records_ok(bool asking, int n_top_max, const float* lp, const int32_t* ids, const float* lps)
{
    if (n_top_max < 0 || n_top_max > GTEN_HIP_LOGPROBS_TOP) return false;
    if (asking && (!lp || (n_top_max > 0 && (!ids || !lps)))) return false;
    return true;
}
// ... and those outputs as the flows take them
inline RecordRows record_rows(bool asking, int n_top_max, float* lp, int32_t* ids, float* lps)
{
    return asking ? RecordRows{lp, ids, lps, n_top_max} : RecordRows{};
}

// a null gten_host_penalties: no penalty
inline const gten_host_penalties& penalties_or_none(const gten_host_penalties* pen)
{
    static const gten_host_penalties none = {nullptr, nullptr, nullptr, nullptr, nullptr, 1.f, 0.f, 0.f, 0, 1};
    return pen ? *pen : none;
}

// one sequence's request from the scalar arguments of the single-sequence exports (a penalty's values for all are the sequence's)
inline Request request_of(int top_k, float temp, uint64_t seed, uint32_t stream, int table = -1, int min_new = 0, int n_top = -1, float top_p = 1.f,
                          float min_p = 0.f, const gten_host_penalties* pen = nullptr, int fsm_start = -1, float miro_tau = 0.f, float miro_eta = 0.1f)
{
    const gten_host_penalties& p = penalties_or_none(pen);
    Request r{top_k, temp, seed, stream, table, min_new, n_top, top_p, min_p, p.rep_all, p.freq_all, p.pres_all, p.last_n_all, p.count_prompt_all != 0, fsm_start};
    r.miro_tau = miro_tau;
    r.miro_eta = miro_eta;
    return r;
}

// the requests of a batch's sequences or a queue's prompts from the list arguments of the batch exports (each list may be null)
inline Requests requests_of(const int32_t* top_k, int top_k_all, const float* temp, float temp_all, uint64_t seed, const uint32_t* stream,
                            const int32_t* table = nullptr, const int32_t* min_new = nullptr, const int32_t* n_top = nullptr, const float* top_p = nullptr,
                            float top_p_all = 1.f, const float* min_p = nullptr, float min_p_all = 0.f, const gten_host_penalties* pen = nullptr,
                            const int32_t* fsm_start = nullptr, const float* miro_tau = nullptr, float miro_tau_all = 0.f, const float* miro_eta = nullptr,
                            float miro_eta_all = 0.1f)
{
    const gten_host_penalties& p = penalties_or_none(pen);
    return Requests::of(top_k, top_k_all, temp, temp_all, seed, stream, table, min_new, n_top, top_p, top_p_all, min_p, min_p_all)
        .penalised(p.rep, p.rep_all, p.freq, p.freq_all, p.pres, p.pres_all, p.last_n, p.last_n_all, p.count_prompt, p.count_prompt_all)
        .bound_to(fsm_start)
        .with_mirostat(miro_tau, miro_tau_all, miro_eta, miro_eta_all);
}

} // namespace gten
