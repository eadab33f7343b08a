// capi_embed.cpp -- flat C exports of include/gten_host_embed.h: the plan (host/embed_plan.h), every text's final-norm rows, and one
// pooled vector per text (host/embed.h).  Kept apart from capi.cpp: this is the only translation unit of the library that names the
// device entry point of include/gten_hip_embed.h.  Every argument is checked before anything is launched.
#include "../../include/gten_host_embed.h"

#include <vector>

#include "capi_handles.h"
#include "embed.h"

using namespace gten;

static_assert(GTEN_HOST_POOL_MEAN == GTEN_HIP_POOL_MEAN && GTEN_HOST_POOL_LAST == GTEN_HIP_POOL_LAST, "one set of pooling codes");

namespace {

thread_local const char* g_why = "";

int refuse(const char* why)
{
    g_why = why;
    return -1;
}

} // namespace

extern "C" {

const char* gten_host_embed_last_error(void) { return g_why; }

int gten_host_embed_plan(const int32_t* lengths, int n_texts, int seg_ok, int32_t* group_of, int32_t* alone)
{
    return embed_plan(lengths, n_texts, seg_ok != 0, group_of, alone);
}

int gten_host_model_hidden_many(gten_host_model* m, const int32_t* tokens, const int32_t* starts, int n_texts, int layer,
                                void* rows_out, int* dtype_out)
{
    g_why = "";
    if (!m) return refuse("hidden_many: null model");
    std::vector<int> lengths;
    if (const char* why = embed_texts_ok(*m->model, tokens, starts, n_texts, layer, &lengths)) return refuse(why);
    if (!rows_out || !dtype_out) return refuse("hidden_many: null output");
    *dtype_out = hidden_many(*m->model, tokens, starts, lengths, layer, (uint8_t*)rows_out);
    return 0;
}

int gten_host_model_embed_many(gten_host_model* m, const int32_t* tokens, const int32_t* starts, int n_texts, int pooling,
                               int normalize, int layer, float* out)
{
    g_why = "";
    if (!m) return refuse("embed_many: null model");
    std::vector<int> lengths;
    if (const char* why = embed_texts_ok(*m->model, tokens, starts, n_texts, layer, &lengths)) return refuse(why);
    if (pooling != GTEN_HOST_POOL_MEAN && pooling != GTEN_HOST_POOL_LAST) return refuse("embed_many: unknown pooling");
    if (!out) return refuse("embed_many: null output");
    embed_many(*m->model, tokens, starts, lengths, pooling, normalize != 0, layer, out);
    return 0;
}

} // extern "C"
