// embed.h -- the hidden states of texts on one TinyLlama: every row in storage form (hidden_many) or one pooled vector per text
// (embed_many).  include/gten_host_embed.h states the contract, host/embed_plan.h decides which texts share a prompt pass, and
// include/gten_hip_embed.h defines the pooling.  Included by host/capi_embed.cpp and the command line program only: nothing else in
// the library names the device entry point.  DESIGN.md 3.22.
#pragma once

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/gten_hip_embed.h"
#include "embed_plan.h"
#include "tinyllama_model.h"

namespace gten {

// the plan restates score_many's grouping: one set of numbers
static_assert(kEmbedGroupTexts == TinyLlama::kScoreTexts && kEmbedGroupRows == TinyLlama::kScoreRows, "embed_plan.h and score_many group alike");

// the checks both calls share (null: fine); fills the texts' lengths.  Nothing has been launched when a text is returned.
inline const char* embed_texts_ok(const TinyLlama& model, const int32_t* tokens, const int32_t* starts, int n_texts, int layer, std::vector<int>* lengths)
{
    if (!tokens || !starts) return "embed: null pointer";
    if (n_texts < 1 || starts[0] != 0) return "embed: no texts, or starts[0] != 0";
    if (layer < 0 || layer > model.params.n_layers) return "embed: layer outside [0, n_layers]";
    const int max_len = std::min(kEmbedGroupMax, model.n_ctx_);
    for (int k = 0; k < n_texts; k++) {
        const long long len = (long long)starts[k + 1] - starts[k];
        if (len < 1) return "embed: an empty text";
        if (len > max_len) return "embed: a text over min(2048, max_ctx) ids";
        lengths->push_back((int)len);
    }
    for (int i = 0; i < starts[n_texts]; i++)
        if (tokens[i] < 0 || tokens[i] >= model.params.n_vocab) return "embed: an id outside [0, n_vocab)";
    return nullptr;
}

// the prompt passes of the plan: fn(texts of the group in order, its rows' tensor, starts inside it) once per group, in order.
// Grouped texts run on the model's segmented-prompt twin (hidden_rows), a text that goes alone on the model itself (final_rows).
template <class Fn>
void embed_for_each_group(TinyLlama& model, const int32_t* tokens, const int32_t* starts, const std::vector<int>& lengths, int layer, Fn fn)
{
    const TinyLLamaParams& p = model.params;
    const int n_texts = (int)lengths.size();
    const int n_blocks = layer == 0 ? p.n_layers : layer;
    const bool seg = gten_hip_row_segments_ok(p.n_embd, p.n_ffn, p.n_heads, p.n_query_groups, dtype_code(model.dtype_.wdtype),
                                              dtype_code(model.dtype_.adtype)) == 1;
    std::vector<int> group_of((size_t)n_texts), alone((size_t)n_texts);
    const int n_groups = embed_plan(lengths.data(), n_texts, seg, group_of.data(), alone.data());
    std::vector<std::vector<int>> members((size_t)n_groups);
    for (int k = 0; k < n_texts; k++) members[(size_t)group_of[(size_t)k]].push_back(k);
    for (int g = 0; g < n_groups; g++) {
        std::vector<int32_t> ids, st{0};
        for (int k : members[(size_t)g]) {
            ids.insert(ids.end(), tokens + starts[k], tokens + starts[k + 1]);
            st.push_back((int32_t)ids.size());
        }
        Tensor tk(ids.data(), {(int)ids.size()}, kInt32);
        const Tensor h = alone[(size_t)g] ? model.final_rows(tk, 0, n_blocks) : model.segment_model().hidden_rows(tk, st, n_blocks);
        fn(members[(size_t)g], h, st);
    }
}

// rows_out: starts[n_texts] rows of gten_hip_row_bytes(activation dtype, n_embd) bytes; returns the dtype code
inline int hidden_many(TinyLlama& model, const int32_t* tokens, const int32_t* starts, const std::vector<int>& lengths, int layer, uint8_t* rows_out)
{
    const int dt = dtype_code(model.dtype_.adtype);
    const size_t rb = gten_hip_row_bytes(dt, model.params.n_embd);
    std::vector<uint8_t> stage;
    embed_for_each_group(model, tokens, starts, lengths, layer, [&](const std::vector<int>& texts, const Tensor& h, const std::vector<int32_t>& st) {
        const size_t pitch = (size_t)h.bstride(0);
        stage.resize((size_t)st.back() * pitch);
        GTEN_HIP_OK(gten_hip_memcpy_d2h(stage.data(), h.device_ptr(), stage.size()));
        for (size_t i = 0; i < texts.size(); i++)
            for (int r = 0; r < st[i + 1] - st[i]; r++)
                std::memcpy(rows_out + (size_t)(starts[texts[i]] + r) * rb, stage.data() + (size_t)(st[i] + r) * pitch, rb);
    });
    return dt;
}

// the pooled vectors of one call, in the plan's order: ONE device buffer per process, grown on demand and never released, shared by
// every model.  Fine for the callers there are -- one calling thread, each call synchronous (it ends in the copy back) -- and stated
// as a restriction in include/gten_host_embed.h.
inline float* embed_vec_scratch(size_t bytes)
{
    static float* vec = nullptr;
    static size_t cap = 0;
    if (bytes > cap) {
        if (vec) GTEN_HIP_OK(gten_hip_free(vec));
        vec = nullptr;
        cap = 0;
        void* p = nullptr;
        GTEN_HIP_OK(gten_hip_malloc(&p, bytes));
        vec = (float*)p;
        cap = bytes;
    }
    return vec;
}

// out: f32 [n_texts][n_embd] on the host.  One gten_hip_pool_rows call per group while its rows are on the device, one copy back.
inline void embed_many(TinyLlama& model, const int32_t* tokens, const int32_t* starts, const std::vector<int>& lengths, int pooling, bool normalize,
                       int layer, float* out)
{
    const size_t E = (size_t)model.params.n_embd, n_texts = lengths.size();
    float* vec = embed_vec_scratch(n_texts * E * sizeof(float));
    std::vector<int> order;                                   // the text behind each vector of `vec`
    embed_for_each_group(model, tokens, starts, lengths, layer, [&](const std::vector<int>& texts, const Tensor& h, const std::vector<int32_t>& st) {
        GTEN_HIP_OK(gten_hip_pool_rows(h.device_ptr(), dtype_code(h.dtype()), (size_t)h.bstride(0), (int)E, st.data(), (int)texts.size(), pooling,
                                       normalize ? 1 : 0, vec + order.size() * E));
        order.insert(order.end(), texts.begin(), texts.end());
    });
    std::vector<float> got(n_texts * E);
    GTEN_HIP_OK(gten_hip_memcpy_d2h(got.data(), vec, got.size() * sizeof(float)));
    for (size_t i = 0; i < order.size(); i++) std::memcpy(out + (size_t)order[i] * E, got.data() + i * E, E * sizeof(float));
}

} // namespace gten
