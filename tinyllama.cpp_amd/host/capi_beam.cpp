// capi_beam.cpp -- flat C exports of beam search (include/gten_host_beam.h).  Kept apart from capi.cpp like capi_sessions.cpp: this
// is the only translation unit that refers to the device entry points of include/gten_hip_beam.h (through host/beam_search.h).
#include "../../include/gten_host_beam.h"

#include <cstring>

#include "capi_handles.h"
#include "beam_search.h"

using namespace gten;

static_assert(kBeamMax == GTEN_HOST_BEAM_MAX && sizeof(BeamState) == GTEN_HOST_BEAM_STATE_BYTES, "host/beam_plan.h and include/gten_host_beam.h disagree");
static_assert(kBeamEndedEos == GTEN_HOST_BEAM_ENDED_EOS && kBeamEndedLength == GTEN_HOST_BEAM_ENDED_LENGTH, "ended_by codes");

namespace {

// `hyp` (at most n_beams of them) into the flat outputs of one prompt; a hypothesis longer than max_new is cut (there is none)
void hyp_out(const std::vector<BeamHypothesis>& hyp, int max_new, int32_t* ids_out, int32_t* n_ids_out, float* final_out, float* cum_out, int32_t* ended_by_out)
{
    for (size_t i = 0; i < hyp.size(); i++) {
        const size_t n = std::min(hyp[i].ids.size(), (size_t)max_new);
        if (ids_out && n) std::memcpy(ids_out + i * (size_t)max_new, hyp[i].ids.data(), n * sizeof(int32_t));
        if (n_ids_out) n_ids_out[i] = (int32_t)n;
        if (final_out) final_out[i] = hyp[i].final_score;
        if (cum_out) cum_out[i] = hyp[i].cum;
        if (ended_by_out) ended_by_out[i] = hyp[i].ended_by;
    }
}

} // namespace

extern "C" {

int gten_host_batch_beam_search(gten_host_batch* b, const int32_t* tokens, const int32_t* starts, int n_prompts, int n_beams, int max_new, int eos,
                                float length_penalty, int32_t* ids_out, int32_t* n_ids_out, float* final_out, float* cum_out, int32_t* ended_by_out,
                                int32_t* n_hyp, int* rounds_out)
{
    if (!b || !tokens || !starts || n_prompts < 1 || n_beams < 1 || max_new < 1 || !n_hyp) return -1;
    std::vector<std::vector<int32_t>> prompts((size_t)n_prompts);
    for (int g = 0; g < n_prompts; g++) {
        if (starts[g + 1] <= starts[g]) return -1;
        prompts[(size_t)g].assign(tokens + starts[g], tokens + starts[g + 1]);
        for (int32_t id : prompts[(size_t)g])
            if (id < 0 || id >= b->cfg.n_vocab) return -1;
    }
    std::vector<std::vector<BeamHypothesis>> out;
    if (int rc = beam_search(*b->batch, prompts, n_beams, max_new, eos, length_penalty, &out, rounds_out)) return rc;
    for (int g = 0; g < n_prompts; g++) {
        const size_t at = (size_t)g * (size_t)n_beams;
        n_hyp[g] = (int32_t)out[(size_t)g].size();
        hyp_out(out[(size_t)g], max_new, ids_out ? ids_out + at * (size_t)max_new : nullptr, n_ids_out ? n_ids_out + at : nullptr, final_out ? final_out + at : nullptr,
                cum_out ? cum_out + at : nullptr, ended_by_out ? ended_by_out + at : nullptr);
    }
    return 0;
}

int gten_host_beam_weights(int max_new, float length_penalty, float* w_out)
{
    if (max_new < 0 || !w_out) return -1;
    const std::vector<float> w = beam_weights(max_new, length_penalty);
    std::memcpy(w_out, w.data(), w.size() * sizeof(float));
    return 0;
}

int gten_host_beam_backtrack(const int32_t* parent, const int32_t* ids, int rows, int t, int b, int32_t* out)
{
    if (rows < 0 || t < 0 || t > rows || b < 0 || b >= kBeamMax || (t > 0 && (!parent || !ids || !out))) return -1;
    const std::vector<int32_t> got = beam_backtrack(BeamTrellis{parent, ids, rows}, t, b);
    if ((int)got.size() != t) return -1;
    if (t) std::memcpy(out, got.data(), got.size() * sizeof(int32_t));
    return t;
}

int gten_host_beam_finalize(const void* state, const int32_t* parent, const int32_t* ids, int rows, int n_beams, const float* w, int max_new, int32_t* ids_out,
                            int32_t* n_ids_out, float* final_out, float* cum_out, int32_t* ended_by_out)
{
    if (!state || !w || n_beams < 1 || n_beams > kBeamMax || max_new < 1 || rows < 0) return -1;
    BeamState st;
    std::memcpy(&st, state, sizeof(st));
    if (st.t < 0 || st.t > rows || st.t > max_new || (rows > 0 && (!parent || !ids))) return -1;
    const std::vector<BeamHypothesis> hyp = beam_finalize(st, BeamTrellis{parent, ids, rows}, n_beams, w);
    hyp_out(hyp, max_new, ids_out, n_ids_out, final_out, cum_out, ended_by_out);
    return (int)hyp.size();
}

} // extern "C"
