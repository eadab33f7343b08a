// capi_fsm.cpp -- flat C exports of include/gten_host_fsm.h: the automaton builders of host/fsm_build.h and generation bound to a token
// automaton (host/generate.h's flows with all six stages -- the only instantiation of kFsm in the library).
#include "../../include/gten_host_fsm.h"

#include <vector>

#include "../../include/gten_hip_regex.h"
#include "../../include/gten_hip_stoptext.h"
#include "capi_handles.h"
#include "fsm_build.h"

using namespace gten;

namespace {

constexpr unsigned kAll = kSampled | kBiased | kLogprobs | kNucleus | kPenalty | kFsm;
const gten_host_penalties kNone = {nullptr, nullptr, nullptr, nullptr, nullptr, 1.f, 0.f, 0.f, 0, 1};

bool records_ok(bool asking, int n_top_max, const float* lp, const int32_t* ids, const float* lps)
{
    if (n_top_max < 0 || n_top_max > GTEN_HIP_LOGPROBS_TOP) return false;
    if (asking && (!lp || (n_top_max > 0 && (!ids || !lps)))) return false;
    return true;
}

Requests with(const Requests& r, const gten_host_penalties* pen, const int32_t* fsm_start)
{
    const gten_host_penalties& p = pen ? *pen : kNone;
    return r.penalised(p.rep, p.rep_all, p.freq, p.freq_all, p.pres, p.pres_all, p.last_n, p.last_n_all, p.count_prompt, p.count_prompt_all).bound_to(fsm_start);
}

int set_pool(gten_hip_decoder* dec, int n_vocab, const gten_host_fsm* f)
{
    if (!f) return gten_hip_decoder_set_fsm(dec, nullptr, nullptr, 0);
    if (f->pool.n_vocab() != n_vocab || f->pool.n_states() < 1) return -1;
    if (f->pool.has_regex()) {
        // regex ranges never cross the bus as tables: the decoder gets the vocabulary's bytes and expands them itself
        // (include/gten_hip_regex.h); the ranges of host rows are uploaded as they always were
        if (const int rc = gten_hip_decoder_set_vocab_bytes(dec, f->pool.vocab_bytes(), f->pool.vocab_offsets())) return rc;
        // (a search range -- stop strings as text, include/gten_hip_stoptext.h -- goes the same way under its own mode)
        std::vector<gten_hip_fsm_part_ex> parts;
        for (const FsmPool::Part& p : f->pool.parts()) {
            if (p.regex < 0) {
                parts.push_back(gten_hip_fsm_part_ex{p.first, p.count, f->pool.host_rows(p), nullptr, nullptr, 0, -1, GTEN_HIP_FSM_PART_MATCH});
            } else {
                const FsmPool::Regex& r = f->pool.regex(p.regex);
                parts.push_back(gten_hip_fsm_part_ex{p.first, p.count, nullptr, r.dfa.next.data(), r.dfa.accept.data(), r.dfa.n_states(), r.eos,
                                                     r.mode == FsmPool::kSearch ? GTEN_HIP_FSM_PART_SEARCH : GTEN_HIP_FSM_PART_MATCH});
            }
        }
        return gten_hip_decoder_set_fsm_parts_ex(dec, f->pool.n_states(), f->pool.flags(), parts.data(), (int)parts.size());
    }
    return gten_hip_decoder_set_fsm(dec, f->pool.next(), f->pool.flags(), f->pool.n_states());
}

int info(gten_hip_decoder* dec, int* n_states, int32_t* state, int32_t* pos)
{
    int on = 0;
    if (gten_hip_decoder_fsm_info(dec, n_states, state, pos, &on, 0, 0, 0, nullptr, nullptr, nullptr)) return -1;
    return on;
}

} // namespace

extern "C" {

gten_host_fsm* gten_host_fsm_create(int n_vocab)
{
    if (n_vocab < 1 || n_vocab > 65535) return nullptr;
    return new gten_host_fsm{FsmPool(n_vocab)};
}

void gten_host_fsm_free(gten_host_fsm* f) { delete f; }

int gten_host_fsm_add_stop(gten_host_fsm* f, const int32_t* ids, const int32_t* offsets, int n) { return f ? f->pool.add_stop(ids, offsets, n) : -1; }

int gten_host_fsm_add_choices(gten_host_fsm* f, const int32_t* ids, const int32_t* offsets, int n) { return f ? f->pool.add_choices(ids, offsets, n) : -1; }

int gten_host_fsm_add_table(gten_host_fsm* f, const uint16_t* next, const uint8_t* flags, int n_states)
{
    return f ? f->pool.add_table(next, flags, n_states) : -1;
}

int gten_host_fsm_n_states(const gten_host_fsm* f) { return f ? f->pool.n_states() : -1; }

int gten_host_fsm_tables(const gten_host_fsm* f, const uint16_t** next, const uint8_t** flags)
{
    if (!f) return -1;
    if (next) *next = f->pool.next();
    if (flags) *flags = f->pool.flags();
    return f->pool.n_states();
}

int gten_host_model_set_fsm(gten_host_model* m, const gten_host_fsm* f)
{
    if (!m) return -1;
    return set_pool(m->model->decoder_handle(), m->cfg.n_vocab, f);
}

int gten_host_batch_set_fsm(gten_host_batch* b, const gten_host_fsm* f)
{
    if (!b) return -1;
    return set_pool(b->batch->decoder_handle(), b->cfg.n_vocab, f);
}

int gten_host_model_fsm_info(gten_host_model* m, int* n_states, int32_t* state_out, int32_t* pos_out)
{
    if (!m) return -1;
    return info(m->model->decoder_handle(), n_states, state_out, pos_out);
}

int gten_host_batch_fsm_info(gten_host_batch* b, int* n_states, int32_t* state_out, int32_t* pos_out)
{
    if (!b) return -1;
    return info(b->batch->decoder_handle(), n_states, state_out, pos_out);
}

int gten_host_model_set_seq_fsm(gten_host_model* m, int state, int pos)
{
    if (!m) return -1;
    return gten_hip_decoder_set_seq_fsm(m->model->decoder_handle(), 0, state, pos);
}

int gten_host_batch_set_seq_fsm(gten_host_batch* b, int seq, int state, int pos)
{
    if (!b) return -1;
    return gten_hip_decoder_set_seq_fsm(b->batch->decoder_handle(), seq, state, pos);
}

int gten_host_model_fsm_states(gten_host_model* m, int from, int count, int32_t* states_out)
{
    if (!m) return -1;
    return gten_hip_decoder_slot_states(m->model->decoder_handle(), 0, from, count, states_out);
}

int gten_host_batch_fsm_states(gten_host_batch* b, int seq, int from, int count, int32_t* states_out)
{
    if (!b) return -1;
    return gten_hip_decoder_slot_states(b->batch->decoder_handle(), seq, from, count, states_out);
}

void* gten_host_batch_fsm_decoder(gten_host_batch* b) { return b ? (void*)b->batch->decoder_handle() : nullptr; }

int gten_host_model_generate_fsm(gten_host_model* m, int32_t* tokens, int n_prompt, int max_tokens, int eos, int top_k, float temp, uint64_t seed,
                                 uint32_t stream, int table, int min_new, int n_top, float top_p, float min_p, float* logprob_out, int32_t* top_id_out,
                                 float* top_logprob_out, const gten_host_penalties* pen, int fsm_start, int32_t* ended_by)
{
    if (!m || !tokens || n_prompt <= 0 || max_tokens <= 0 || !request_ok(top_k, temp) || !binding_ok(table, min_new) || !cut_ok(top_p, min_p)) return -1;
    if (n_top < -1 || !records_ok(n_top >= 0, std::max(n_top, 0), logprob_out, top_id_out, top_logprob_out)) return -1;
    const gten_host_penalties& p = pen ? *pen : kNone;
    if (!penalty_ok(p.rep_all, p.freq_all, p.pres_all, p.last_n_all) || !fsm_ok(fsm_start, table)) return -1;
    const RecordRows rows = n_top >= 0 ? RecordRows{logprob_out, top_id_out, top_logprob_out, n_top} : RecordRows{};
    const Request r{top_k, temp, seed, stream, table, min_new, n_top, top_p, min_p, p.rep_all, p.freq_all, p.pres_all, p.last_n_all, p.count_prompt_all != 0,
                    fsm_start};
    int ended = kEndedByLength;
    const int total = generate_in_place<kAll>(*m->model, tokens, n_prompt, max_tokens, eos, r, rows, &ended, m->cfg.max_ctx);
    if (ended_by) *ended_by = ended;
    return total;
}

int gten_host_batch_generate_fsm(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int max_prompt, int max_tokens, int eos,
                                 const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed, const uint32_t* stream,
                                 const int32_t* table, const int32_t* min_new, int32_t* out, int32_t* n_total, const int32_t* n_top, int n_top_max,
                                 float* logprob_out, int32_t* top_id_out, float* top_logprob_out, const float* top_p, const float* min_p,
                                 float top_p_all, float min_p_all, const gten_host_penalties* pen, const int32_t* fsm_start, int32_t* ended_by)
{
    if (!b || !prompts || !n_prompt || !out || !n_total || max_tokens <= 0) return -1;
    if (!records_ok(n_top != nullptr, n_top_max, logprob_out, top_id_out, top_logprob_out)) return -1;
    const RecordRows rows = n_top ? RecordRows{logprob_out, top_id_out, top_logprob_out, n_top_max} : RecordRows{};
    return generate_batch<kAll>(*b->batch, b->cfg.max_ctx, prompts, n_prompt, max_prompt, max_tokens, eos,
                                with(Requests::of(top_k, top_k_all, temp, temp_all, seed, stream, table, min_new, n_top, top_p, top_p_all, min_p, min_p_all), pen,
                                     fsm_start),
                                out, n_total, rows, ended_by);
}

int gten_host_batch_serve_fsm(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int n_prompts, int max_prompt, int max_tokens,
                              int eos, int slice, int max_new, const int32_t* max_new_each, int32_t* out, int32_t* n_total, double* stats, int n_stats,
                              const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed, const int32_t* table,
                              const int32_t* min_new, const int32_t* n_top, int n_top_max, float* logprob_out, int32_t* top_id_out,
                              float* top_logprob_out, const float* top_p, const float* min_p, float top_p_all, float min_p_all,
                              const gten_host_penalties* pen, const int32_t* fsm_start, int32_t* ended_by)
{
    if (!b || !prompts || !n_prompt || !out || !n_total || n_prompts <= 0 || max_prompt <= 0 || n_stats < 0 || (n_stats > 0 && !stats)) return -1;
    if (max_tokens <= 0 || slice <= 0) return -1;
    if (!records_ok(n_top != nullptr, n_top_max, logprob_out, top_id_out, top_logprob_out)) return -1;
    const RecordRows rows = n_top ? RecordRows{logprob_out, top_id_out, top_logprob_out, n_top_max} : RecordRows{};
    return serve_queue<kAll>(*b->batch, b->cfg.max_ctx, prompts, n_prompt, n_prompts, max_prompt, max_tokens, eos, slice, max_new, max_new_each, out, n_total,
                             stats, n_stats,
                             with(Requests::of(top_k, top_k_all, temp, temp_all, seed, nullptr, table, min_new, n_top, top_p, top_p_all, min_p, min_p_all), pen,
                                  fsm_start),
                             rows, ended_by);
}

} // extern "C"
