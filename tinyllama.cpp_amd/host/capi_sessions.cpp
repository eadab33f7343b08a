// capi_sessions.cpp -- flat C exports of continued sequences (include/gten_host_sessions.h).  Kept apart from capi.cpp: this is
// the only translation unit that refers to the continued device entry points (include/gten_hip_continue.h); it hands them
// to the headers' hook (gten/modules.h, detail::continued_rows) when the library is loaded.
#include "../../include/gten_host_sessions.h"
#include "../../include/gten_hip_continue.h"

#include <algorithm>

#include "capi_handles.h"
#include "session_plan.h"

using namespace gten;

namespace {

const bool installed = [] {
    detail::continued_rows().set = gten_hip_set_row_contexts;
    detail::continued_rows().call = gten_hip_block_rows_continued;
    return true;
}();

constexpr unsigned kAll = kSampled | kBiased | kLogprobs | kNucleus | kPenalty | kFsm;
const gten_host_penalties kNone = {nullptr, nullptr, nullptr, nullptr, nullptr, 1.f, 0.f, 0.f, 0, 1};

} // namespace

static_assert(TinyLlamaBatch::kSessionsMax == GTEN_HOST_SESSIONS_MAX, "host/tinyllama_model.h and include/gten_host_sessions.h disagree");

extern "C" {

int gten_host_batch_sessions_reserve(gten_host_batch* b, int n) { return b ? b->batch->sessions_reserve(n) : -1; }
int gten_host_batch_session_open(gten_host_batch* b) { return b ? b->batch->session_open() : -1; }
int gten_host_batch_session_close(gten_host_batch* b, int id) { return b ? b->batch->session_close(id) : -1; }

int gten_host_batch_session_info(gten_host_batch* b, int id, int* n_ids, int* rows, int* prefix_which, int* prefix_rows)
{
    if (!b || !b->batch->session_is_open(id)) return -1;
    int w = -1, p = 0;
    b->batch->session_prefix(id, &w, &p);
    if (n_ids) *n_ids = (int)b->batch->session_ids(id).size();
    if (rows) *rows = b->batch->session_rows(id);
    if (prefix_which) *prefix_which = w;
    if (prefix_rows) *prefix_rows = p;
    return 0;
}

int gten_host_batch_session_ids(gten_host_batch* b, int id, int32_t* out, int n)
{
    if (!b || !b->batch->session_is_open(id) || n < 0 || (n > 0 && !out)) return -1;
    const std::vector<int32_t>& ids = b->batch->session_ids(id);
    std::copy(ids.begin(), ids.begin() + std::min((size_t)n, ids.size()), out);
    return (int)ids.size();
}

int gten_host_batch_session_truncate(gten_host_batch* b, int id, int n_ids) { return b ? b->batch->session_truncate(id, n_ids) : -1; }

int gten_host_batch_sessions_info(gten_host_batch* b, int* open, unsigned long long* kv_bytes_per_session, unsigned long long* turns,
                                  unsigned long long* turns_continued, unsigned long long* rows_computed, unsigned long long* rows_kept)
{
    if (!b) return -1;
    b->batch->sessions_info(open, kv_bytes_per_session, turns, turns_continued, rows_computed, rows_kept);
    return 0;
}

int gten_host_batch_serve_sessions(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int n_prompts, int max_prompt, int max_tokens,
                                   int eos, int slice, int max_new, const int32_t* max_new_each, int32_t* out, int32_t* n_total, double* stats, int n_stats,
                                   const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed, const int32_t* table,
                                   const int32_t* min_new, const int32_t* n_top, int n_top_max, float* logprob_out, int32_t* top_id_out,
                                   float* top_logprob_out, const float* top_p, const float* min_p, float top_p_all, float min_p_all,
                                   const gten_host_penalties* pen, const int32_t* fsm_start, int32_t* ended_by, const int32_t* session)
{
    if (!b || !prompts || !n_prompt || !out || !n_total || n_prompts <= 0 || max_prompt <= 0 || n_stats < 0 || (n_stats > 0 && !stats) || !installed) return -1;
    if (max_tokens <= 0 || slice <= 0) return -1;
    if (n_top_max < 0 || n_top_max > GTEN_HIP_LOGPROBS_TOP) return -1;
    if (n_top && (!logprob_out || (n_top_max > 0 && (!top_id_out || !top_logprob_out)))) return -1;
    const gten_host_penalties& p = pen ? *pen : kNone;
    const Requests reqs = Requests::of(top_k, top_k_all, temp, temp_all, seed, nullptr, table, min_new, n_top, top_p, top_p_all, min_p, min_p_all)
                              .penalised(p.rep, p.rep_all, p.freq, p.freq_all, p.pres, p.pres_all, p.last_n, p.last_n_all, p.count_prompt, p.count_prompt_all)
                              .bound_to(fsm_start);
    const RecordRows rows = n_top ? RecordRows{logprob_out, top_id_out, top_logprob_out, n_top_max} : RecordRows{};
    return serve_queue<kAll>(*b->batch, b->cfg.max_ctx, prompts, n_prompt, n_prompts, max_prompt, max_tokens, eos, slice, max_new, max_new_each, out, n_total,
                             stats, n_stats, reqs, rows, ended_by, nullptr, session);
}

int gten_host_batch_extend_many(gten_host_batch* b, const int32_t* seqs, const int32_t* ctx_len, const int32_t* tokens, const int32_t* starts, int n,
                                float* logits_out, int32_t* first_out)
{
    if (!b || !seqs || !ctx_len || !tokens || !starts || n < 1 || starts[0] != 0 || !installed) return -1;
    TinyLlamaBatch& batch = *b->batch;
    std::vector<char> seen((size_t)batch.n_seq(), 0);
    std::vector<int> sq, ctx;
    std::vector<std::vector<int32_t>> tails((size_t)n);
    std::vector<float*> lo;
    for (int k = 0; k < n; k++) {
        const int len = starts[k + 1] - starts[k];
        if (seqs[k] < 0 || seqs[k] >= batch.n_seq() || seen[(size_t)seqs[k]]) return -1;
        if (ctx_len[k] < 1 || len < 1 || ctx_len[k] + len > batch.max_ctx()) return -1;
        seen[(size_t)seqs[k]] = 1;
        sq.push_back(seqs[k]);
        ctx.push_back(ctx_len[k]);
        tails[(size_t)k].assign(tokens + starts[k], tokens + starts[k + 1]);
        lo.push_back(logits_out ? logits_out + (size_t)k * (size_t)b->cfg.n_vocab : nullptr);
    }
    std::vector<int> first;
    batch.extend_many(sq, ctx, tails, &first, &lo);
    if (first_out)
        for (int k = 0; k < n; k++) first_out[k] = first[(size_t)k];
    return 0;
}

int gten_host_batch_extend_info(gten_host_batch* b, unsigned long long* turns_continued, unsigned long long* rows_computed,
                                unsigned long long* rows_kept, unsigned long long* rows_one_by_one)
{
    if (!b) return -1;
    b->batch->extend_info(turns_continued, rows_computed, rows_kept, rows_one_by_one);
    return 0;
}

int gten_host_session_plan(int n_ids, int rows, int n_new, int segmented, int* ctx, int* compute, int* path)
{
    SessionPlan p;
    if (!session_plan(n_ids, rows, n_new, segmented != 0, &p)) return -1;
    if (ctx) *ctx = p.ctx;
    if (compute) *compute = p.rows;
    if (path) *path = p.path;
    return 0;
}

} // extern "C"
