// beam_search.h -- beam search as a fixed-batch call on a TinyLlamaBatch: G prompts x B beams on sequences
// g * B .. g * B + B - 1 of the batch, the other sequences idle.  Each prompt is processed once and fanned out to its beams' cache
// sets; every round is one shared step of the batch's decoder, the decision and the K / V gather on the device
// (include/gten_hip_beam.h); one word per round comes back.  Included by host/capi_beam.cpp only.
#pragma once

#include "../../include/gten_hip_beam.h"

#include "beam_plan.h"
#include "tinyllama_model.h"

namespace gten {

static_assert(kBeamMax == GTEN_HIP_BEAM_MAX && sizeof(BeamState) == sizeof(gten_hip_beam_state), "host/beam_plan.h and include/gten_hip_beam.h disagree");

// 0 and out[g] = group g's hypotheses, best first; -1: bad arguments; otherwise the device's refusal (gten_hip_last_error()).
// rounds_out: the rounds that ran (the loop ends early once every group is done).
inline int beam_search(TinyLlamaBatch& batch, const std::vector<std::vector<int32_t>>& prompts, int n_beams, int max_new, int eos, float length_penalty,
                       std::vector<std::vector<BeamHypothesis>>* out, int* rounds_out = nullptr)
{
    const int G = (int)prompts.size(), B = n_beams;
    if (G < 1 || !out || max_new < 1 || B < 1) return -1;
    for (const std::vector<int32_t>& p : prompts)
        if (p.empty()) return -1;
    gten_hip_decoder* dec = batch.decoder_handle();
    const std::vector<float> w = beam_weights(max_new, length_penalty);
    std::vector<gten_hip_beam_group> groups((size_t)G);
    for (int g = 0; g < G; g++) groups[(size_t)g] = gten_hip_beam_group{g * B, B, (int)prompts[(size_t)g].size(), max_new, eos};
    // the refusals that need no prompt pass come first: nothing is computed for a search that cannot begin
    for (int g = 0; g < G; g++)
        if (B > GTEN_HIP_BEAM_MAX || (long long)G * B > batch.n_seq() || (long long)prompts[(size_t)g].size() + max_new > batch.max_ctx()) {
            const int rc = gten_hip_decoder_beam_begin(dec, groups.data(), G, w.data(), (int)w.size());
            return rc ? rc : -1;
        }
    // ---- each prompt once, onto beam 0's set, its rows fanned out to the other beams' sets
    auto wide_ok = [&](int g) { return batch.batched_prompts() && (int)prompts[(size_t)g].size() >= 16 && (int)prompts[(size_t)g].size() <= TinyLlamaBatch::kPreRows; };
    std::vector<int> slots, copy_of, first;
    std::vector<const std::vector<int32_t>*> items;
    int rows = 0, computed = 0;
    auto flush = [&]() {
        if (slots.empty()) return;
        batch.prefill_many(slots, items, &first, nullptr, &copy_of);
        slots.clear(); items.clear(); copy_of.clear();
        rows = computed = 0;
    };
    for (int g = 0; g < G; g++) {
        const std::vector<int32_t>& p = prompts[(size_t)g];
        if (wide_ok(g)) {
            if (computed == TinyLlamaBatch::kPreMax || rows + (int)p.size() > TinyLlamaBatch::kPreRows) flush();
            const int at = (int)slots.size();
            for (int b = 0; b < B; b++) {
                slots.push_back(g * B + b);
                items.push_back(&p);
                copy_of.push_back(b == 0 ? -1 : at);
            }
            rows += (int)p.size();
            computed++;
            continue;
        }
        batch.prefill(g * B, p);
        if (B == 1 || p.size() < 2) continue;
        gten_hip_decoder_desc d0, di;
        std::vector<gten_hip_layer_ptrs> L0, Li;
        batch.seq(g * B).describe(&d0, &L0);
        const size_t bytes = (p.size() - 1) * gten_hip_row_bytes(d0.adtype, (d0.n_embd / d0.n_heads) * d0.n_kv_heads);
        std::vector<gten_hip_copy_range> ranges;
        auto send = [&]() {
            if (!ranges.empty()) GTEN_HIP_OK(gten_hip_copy_ranges(ranges.data(), (int)ranges.size()));
            ranges.clear();
        };
        for (int b = 1; b < B; b++) {
            batch.seq(g * B + b).describe(&di, &Li);
            for (size_t l = 0; l < L0.size(); l++) {
                if (ranges.size() + 2 > (size_t)GTEN_HIP_MAX_COPY_RANGES) send();
                ranges.push_back(gten_hip_copy_range{Li[l].kcache, L0[l].kcache, bytes});
                ranges.push_back(gten_hip_copy_range{Li[l].vcache, L0[l].vcache, bytes});
            }
        }
        send();
    }
    flush();
    for (int g = 0; g < G; g++)
        for (int b = 0; b < B; b++) batch.decode_set_tokens(g * B + b, prompts[(size_t)g].data(), 0, (int)prompts[(size_t)g].size());
    // ---- the rounds
    if (int rc = gten_hip_decoder_beam_begin(dec, groups.data(), G, w.data(), (int)w.size())) return rc;
    int rounds = 0, rc = 0;
    for (; rounds < max_new && !rc;) {
        rc = gten_hip_decoder_beam_round(dec);
        if (rc) break;
        rounds++;
        int live = 0;
        rc = gten_hip_decoder_beam_live(dec, &live);
        if (!rc && live == 0) break;
    }
    out->assign((size_t)G, {});
    std::vector<int32_t> parent((size_t)max_new * kBeamMax), ids((size_t)max_new * kBeamMax);
    for (int g = 0; g < G && !rc; g++) {
        gten_hip_beam_state st;
        rc = gten_hip_decoder_beam_read(dec, g, &st, parent.data(), ids.data());
        if (rc) break;
        BeamState hs;
        std::memcpy(&hs, &st, sizeof(hs));
        (*out)[(size_t)g] = beam_finalize(hs, BeamTrellis{parent.data(), ids.data(), hs.t}, B, w.data());
    }
    const int rc_end = gten_hip_decoder_beam_end(dec);
    if (rounds_out) *rounds_out = rounds;
    return rc ? rc : rc_end;
}

} // namespace gten
