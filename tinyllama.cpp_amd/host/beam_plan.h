// beam_plan.h -- what the host decides about a beam search: the length weights the device multiplies with, the
// walk back through a group's trellis, and the ranking of finished and live hypotheses at the end.  Device-free like serve_plan.h:
// the standard library only, so that tests/host_beam_plan.cpp runs it under sanitizers without a GPU.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace gten {

constexpr int kBeamMax = 8;                      // GTEN_HIP_BEAM_MAX

// a group's state as the device keeps it (the device library's beam header: the same 176 bytes, host/capi_beam.cpp asserts it)
struct BeamState {
    float cum[kBeamMax];
    float fin_final[kBeamMax];
    float fin_cum[kBeamMax];
    int32_t fin_t[kBeamMax];
    int32_t fin_beam[kBeamMax];
    int32_t n_fin, done, t;
    int32_t stepped;
};
static_assert(sizeof(BeamState) == 176, "BeamState is the device's 176 bytes");

// rows [1, rows] of a group's trellis: round t's row at index t - 1, kBeamMax entries each
struct BeamTrellis {
    const int32_t* parent;
    const int32_t* ids;
    int rows;
};

enum { kBeamEndedEos = 0, kBeamEndedLength = 1 };

struct BeamHypothesis {
    std::vector<int32_t> ids;                    // the new ids (eos not stored, as in generate)
    float final_score = 0.f;                     // cum * w[t]
    float cum = 0.f;
    int ended_by = kBeamEndedEos;
};

// w[t] = (float)(1 / t^length_penalty) for t in [1, max_new], w[0] = 0: what a hypothesis of t rounds multiplies its sum with
inline std::vector<float> beam_weights(int max_new, float length_penalty)
{
    std::vector<float> w((size_t)std::max(max_new, 0) + 1, 0.f);
    for (int t = 1; t <= max_new; t++) w[(size_t)t] = (float)(1.0 / std::pow((double)t, (double)length_penalty));
    return w;
}

// the ids of beam b after round t (t of them; t == 0: none).  Empty also where t or b lie outside the trellis or a parent does.
inline std::vector<int32_t> beam_backtrack(const BeamTrellis& tr, int t, int b)
{
    std::vector<int32_t> out;
    if (t < 0 || t > tr.rows || b < 0 || b >= kBeamMax) return out;
    out.resize((size_t)t);
    for (int r = t; r >= 1; r--) {
        if (b < 0 || b >= kBeamMax) return std::vector<int32_t>{};
        out[(size_t)r - 1] = tr.ids[(size_t)(r - 1) * kBeamMax + b];
        b = tr.parent[(size_t)(r - 1) * kBeamMax + b];
    }
    return out;
}

// The best n_beams hypotheses of a group, best first.  Finished ones come from the state's slots: the one finished at round t from
// source b is beam b after round t - 1.  A group that is not done contributes its live beams after round state.t (the caller ran
// max_new rounds) with final = cum[b] * w[state.t], ended by length.  Order: final descending; ties: finished before live, then
// the lower slot or beam.
inline std::vector<BeamHypothesis> beam_finalize(const BeamState& st, const BeamTrellis& tr, int n_beams, const float* w)
{
    struct Item { float fin; int live, at; };
    std::vector<Item> items;
    const int B = std::min(std::max(n_beams, 0), kBeamMax), n_fin = std::min(std::max((int)st.n_fin, 0), B);
    for (int s = 0; s < n_fin; s++) items.push_back(Item{st.fin_final[s], 0, s});
    if (!st.done && st.t >= 1)
        for (int b = 0; b < B; b++) items.push_back(Item{st.cum[b] * w[st.t], 1, b});
    std::stable_sort(items.begin(), items.end(), [](const Item& a, const Item& b) {
        if (a.fin != b.fin) return a.fin > b.fin;
        if (a.live != b.live) return a.live < b.live;
        return a.at < b.at;
    });
    std::vector<BeamHypothesis> out;
    for (size_t i = 0; i < items.size() && (int)i < B; i++) {
        const Item& it = items[i];
        BeamHypothesis h;
        h.final_score = it.fin;
        if (it.live) {
            h.ids = beam_backtrack(tr, st.t, it.at);
            h.cum = st.cum[it.at];
            h.ended_by = kBeamEndedLength;
        } else {
            h.ids = beam_backtrack(tr, st.fin_t[it.at] - 1, st.fin_beam[it.at]);
            h.cum = st.fin_cum[it.at];
            h.ended_by = kBeamEndedEos;
        }
        out.push_back(std::move(h));
    }
    return out;
}

} // namespace gten
