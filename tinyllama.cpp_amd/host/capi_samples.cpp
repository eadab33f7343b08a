// capi_samples.cpp -- flat C exports of n samples per prompt (include/gten_host_samples.h).  Kept apart from
// capi.cpp like capi_prefixes.cpp: this is the only translation unit that refers to the device entry points of
// include/gten_hip_groups.h; it hands them to host/tinyllama_model.h's hooks (detail::groups_decode) when the library is loaded.
#include "../../include/gten_host_samples.h"
#include "../../include/gten_hip_groups.h"

#include <algorithm>
#include <numeric>
#include <vector>

#include "capi_handles.h"

using namespace gten;

static_assert(kGroupsMax == GTEN_GROUPS_MAX, "host/tinyllama_model.h and include/gten_hip_groups.h disagree");
static_assert(TinyLlamaBatch::kGroupsCapDefault == GTEN_HOST_GROUPS_CAP_DEFAULT, "host/tinyllama_model.h and include/gten_host_samples.h disagree");

namespace {

const bool installed = [] {
    detail::groups_decode().set = gten_hip_decoder_group_set;
    detail::groups_decode().share = gten_hip_decoder_group_share;
    detail::groups_decode().info = gten_hip_decoder_groups_info;
    return true;
}();

constexpr unsigned kAll = kSampled | kBiased | kLogprobs | kNucleus | kPenalty | kFsm;
const gten_host_penalties kNone = {nullptr, nullptr, nullptr, nullptr, nullptr, 1.f, 0.f, 0.f, 0, 1};

// the rule of gten_host_samples_rank on sums already formed
int rank(const double* sum, const int32_t* n_new, int n, int32_t* order)
{
    if (!sum || !n_new || !order || n < 0) return -1;
    for (int i = 0; i < n; i++)
        if (n_new[i] < 0) return -1;
    std::iota(order, order + n, 0);
    std::stable_sort(order, order + n, [&](int32_t a, int32_t b) {
        if ((n_new[a] > 0) != (n_new[b] > 0)) return n_new[a] > 0;             // a sample without new ids comes last
        if (n_new[a] == 0) return false;                                       // (... several of them: by index)
        return sum[a] / (double)n_new[a] > sum[b] / (double)n_new[b];          // (ties: stable, the lower sample first)
    });
    return 0;
}

} // namespace

extern "C" {

int gten_host_batch_serve_samples(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int n_prompts, int max_prompt, int max_tokens,
                                  int eos, int slice, int max_new, const int32_t* max_new_each, int32_t* out, int32_t* n_total, double* stats, int n_stats,
                                  const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed, const int32_t* table,
                                  const int32_t* min_new, const int32_t* n_top, int n_top_max, float* logprob_out, int32_t* top_id_out,
                                  float* top_logprob_out, const float* top_p, const float* min_p, float top_p_all, float min_p_all,
                                  const gten_host_penalties* pen, const int32_t* fsm_start, int32_t* ended_by, const int32_t* n_samples, int n_samples_all)
{
    if (!b || !prompts || !n_prompt || !out || !n_total || n_prompts <= 0 || max_prompt <= 0 || n_stats < 0 || (n_stats > 0 && !stats) || !installed) return -1;
    if (max_tokens <= 0 || slice <= 0) return -1;
    if (n_top_max < 0 || n_top_max > GTEN_HIP_LOGPROBS_TOP) return -1;
    if (n_top && (!logprob_out || (n_top_max > 0 && (!top_id_out || !top_logprob_out)))) return -1;
    // the expanded queue: prompt j written out n_samples[j] times in a row, each item a member of group j
    std::vector<int32_t> len, group;
    for (int j = 0; j < n_prompts; j++) {
        const int n = n_samples ? n_samples[j] : n_samples_all;
        if (n < 1 || n > GTEN_HOST_SAMPLES_MAX || n_prompt[j] <= 0 || n_prompt[j] > max_prompt) return -1;
        len.insert(len.end(), (size_t)n, n_prompt[j]);
        group.insert(group.end(), (size_t)n, n > 1 ? j : -1);
    }
    const int n_items = (int)len.size();
    std::vector<int32_t> ids((size_t)n_items * (size_t)max_prompt);
    for (int e = 0, j = 0, i = 0; e < n_items; e++) {
        std::copy(prompts + (size_t)j * max_prompt, prompts + (size_t)(j + 1) * max_prompt, ids.begin() + (size_t)e * max_prompt);
        if (++i == (n_samples ? n_samples[j] : n_samples_all)) { j++; i = 0; }
    }
    const gten_host_penalties& p = pen ? *pen : kNone;
    const Requests reqs = Requests::of(top_k, top_k_all, temp, temp_all, seed, nullptr, table, min_new, n_top, top_p, top_p_all, min_p, min_p_all)
                              .penalised(p.rep, p.rep_all, p.freq, p.freq_all, p.pres, p.pres_all, p.last_n, p.last_n_all, p.count_prompt, p.count_prompt_all)
                              .bound_to(fsm_start);
    const RecordRows rows = n_top ? RecordRows{logprob_out, top_id_out, top_logprob_out, n_top_max} : RecordRows{};
    return serve_queue<kAll>(*b->batch, b->cfg.max_ctx, ids.data(), len.data(), n_items, max_prompt, max_tokens, eos, slice, max_new, max_new_each, out, n_total,
                             stats, n_stats, reqs, rows, ended_by, group.data());
}

int gten_host_batch_samples_info(gten_host_batch* b, unsigned long long* copies, unsigned long long* rows_saved, unsigned long long* groups_recorded,
                                 unsigned long long* groups_unrecorded, int* records_now)
{
    if (!b) return -1;
    b->batch->samples_info(copies, rows_saved, groups_recorded, groups_unrecorded, records_now);
    return 0;
}

int gten_host_batch_set_groups_cap(gten_host_batch* b, int cap)
{
    if (!b) return -1;
    b->batch->set_groups_cap(cap);
    return 0;
}

int gten_host_batch_group_decode_set(gten_host_batch* b, int g, int seq, int rows)
{
    if (!b || seq >= b->batch->n_seq() || rows < 0) return -1;
    return b->batch->group_set_rc(g, seq, rows);                       // (a bad record index is the decoder's refusal)
}

int gten_host_batch_group_decode_share(gten_host_batch* b, int seq, int g, int rows)
{
    if (!b || seq < 0 || seq >= b->batch->n_seq() || rows < 0) return -1;
    return b->batch->group_share_rc(seq, g, rows);
}

int gten_host_batch_groups_decode_info(gten_host_batch* b, int seq, int g, int* group_out, int* chunks_out, int* rows, unsigned long long* imports, int* sharers)
{
    if (!b || seq < 0 || seq >= b->batch->n_seq() || g < 0 || g >= kGroupsMax) return -1;
    b->batch->groups_decode_info(seq, g, group_out, chunks_out, rows, imports, sharers);
    return 0;
}

int gten_host_samples_rank(const double* logprob_sum, const int32_t* n_new, int n, int32_t* order) { return rank(logprob_sum, n_new, n, order); }

int gten_host_samples_rank_records(const float* records, int row_len, int n_prompt, const int32_t* n_new, int n, int32_t* order)
{
    if (!records || !n_new || row_len <= 0 || n_prompt < 0 || n < 0) return -1;
    std::vector<double> sum((size_t)n, 0.0);
    for (int i = 0; i < n; i++) {
        if (n_new[i] < 0 || n_prompt + n_new[i] > row_len) return -1;
        for (int t = 0; t < n_new[i]; t++) sum[(size_t)i] += (double)records[(size_t)i * row_len + (size_t)(n_prompt + t)];
    }
    return rank(sum.data(), n_new, n, order);
}

} // extern "C"
