// capi_score.cpp -- flat C exports of include/gten_host_score.h: scoring given ids with the model (TinyLlama::score,
// ::logits_all, ::score_many in host/tinyllama_model.h).  Kept apart from capi.cpp, like capi_sample.cpp: nothing capi.cpp
// instantiates refers to include/gten_hip_score.h.  Every argument is checked before anything is launched.
#include "../../include/gten_host_score.h"

#include <algorithm>

#include "capi_handles.h"

using namespace gten;

namespace {

bool rows_ok(const gten_host_model* m, const int32_t* tokens, int n, int start_pos)
{
    return m && tokens && n >= 1 && n <= m->cfg.max_ctx && start_pos >= 0 && start_pos < n;
}

bool targets_ok(const gten_host_model* m, const int32_t* targets, int count)
{
    if (!targets) return false;
    for (int i = 0; i < count; i++)
        if (targets[i] < -1 || targets[i] >= m->cfg.n_vocab) return false;
    return true;
}

} // namespace

extern "C" {

int gten_host_model_score(gten_host_model* m, const int32_t* tokens, int n, int start_pos, const int32_t* targets,
                          float* logprob_out, int32_t* rank_out)
{
    if (!rows_ok(m, tokens, n, start_pos) || !logprob_out || !targets_ok(m, targets, n - start_pos)) return -1;
    Tensor tk(tokens, {n}, kInt32);
    m->model->score(tk, start_pos, targets, logprob_out, rank_out);
    return 0;
}

int gten_host_model_logits_all(gten_host_model* m, const int32_t* tokens, int n, int start_pos, float* logits_out)
{
    if (!rows_ok(m, tokens, n, start_pos) || !logits_out) return -1;
    Tensor tk(tokens, {n}, kInt32);
    m->model->logits_all(tk, start_pos, logits_out);
    return 0;
}

int gten_host_model_score_many(gten_host_model* m, const int32_t* tokens, const int32_t* starts, int n_texts,
                               const int32_t* targets, float* logprob_out, int32_t* rank_out)
{
    if (!m || !tokens || !starts || n_texts < 1 || !logprob_out || starts[0] != 0) return -1;
    const int max_len = std::min(2048, m->cfg.max_ctx);
    for (int k = 0; k < n_texts; k++) {
        const int len = starts[k + 1] - starts[k];
        if (len < 1 || len > max_len) return -1;
    }
    if (!targets_ok(m, targets, starts[n_texts])) return -1;
    m->model->score_many(tokens, starts, n_texts, targets, logprob_out, rank_out);
    return 0;
}

} // extern "C"
