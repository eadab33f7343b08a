// generate_shift.h -- generation that goes on past the window (include/gten_host_shift.h): host/generate.h's flows
// cut into SEGMENTS.  A segment is one decode_generate call that ends at max_tokens, at eos or with the window full; between two
// segments the plan (host/shift_plan.h) says whether the sequence shifts, the caches are shifted on the device
// (gten_hip_kv_shift, all sequences and layers of a batch in one call), the decoder's token row is set to what the model now
// sees, and what was bound by position is bound again through phi: the draw stream becomes stream + (shifts << 24), the
// penalty window starts at phi(start).  The out row holds every id in generation order.
//
// Included by host/capi_shift.cpp and the command line program only: it names gten_hip_kv_shift, which host/capi.cpp and the
// headers it instantiates must not (they link against the test stand-in of include/gten_hip.h alone).
#pragma once

#include <string>

#include "generate.h"
#include "shift_plan.h"
#include "../../include/gten_hip_shift.h"

namespace gten {

// shift(keep, drop[i]) of cache set sets[i] whose rows [0, rows[i]) are valid: every set and layer in ONE gten_hip_kv_shift call
inline int kv_shift_sets(const std::vector<TinyLlama*>& sets, const std::vector<int>& rows, int keep, const std::vector<int>& drop, ShiftCounts* counts)
{
    if (sets.empty()) return 0;
    std::vector<gten_hip_kv_shift_item> items;
    gten_hip_decoder_desc d{};
    std::vector<gten_hip_layer_ptrs> L;
    for (size_t i = 0; i < sets.size(); i++) {
        sets[i]->describe(&d, &L);                          // (device_ptr_mut: the tensors' host mirrors are stale from here on)
        for (const gten_hip_layer_ptrs& p : L) items.push_back(gten_hip_kv_shift_item{p.kcache, p.vcache, rows[i], keep, drop[i]});
    }
    const int d_head = d.n_embd / d.n_heads, kv_dim = d_head * d.n_kv_heads;
    const size_t pitch = (size_t)sets[0]->block(0).attn.key.acv.bstride(0);
    if (const int rc = gten_hip_kv_shift(items.data(), (int)items.size(), d.adtype, pitch, kv_dim, d_head)) return rc;
    if (counts)
        for (size_t i = 0; i < sets.size(); i++) {
            counts->shifts++;
            counts->rows_moved += (unsigned long long)(rows[i] - keep - drop[i]);
            counts->rows_dropped += (unsigned long long)drop[i];
        }
    return 0;
}

// what a shifting request must not carry, and why (null: nothing)
inline const char* shift_refusal(const Request& r, int n_prompt, int max_ctx)
{
    if (r.table >= 0) return "generate_shifting: a bias table is bound by position (its `until`) and is not carried through a shift: refused with keep >= 0";
    if (r.n_top >= 0) return "generate_shifting: log-prob records are kept per position and are not carried through a shift: refused with keep >= 0";
    if (r.fsm_start >= 0) return "generate_shifting: an automaton's states are kept per position and are not carried through a shift: refused with keep >= 0";
    if (r.miro_tau != 0.f) return "generate_shifting: mirostat's mu is kept per position and is not carried through a shift: refused with keep >= 0";
    if (r.stream >= (1u << 24)) return "generate_shifting: stream >= 2^24 (a shifted sequence draws on stream + (shifts << 24)): refused with keep >= 0";
    if (!shift_ok(max_ctx, r.shift_keep, r.shift_drop)) return "generate_shifting: keep + drop do not fit a full window";
    if (n_prompt >= max_ctx) return "generate_shifting: the prompt fills the window";
    return nullptr;
}

// the requests of a sequence that has shifted `shifts` times: the draw stream, the penalty window's start (already through phi)
template <unsigned M>
int rebind_shifted(gten_hip_decoder* dec, int q, const Request& r, unsigned shifts, int pen_start)
{
    if constexpr ((M & kSampled) != 0)
        if (const int rc = gten_hip_decoder_set_sampling(dec, q, r.top_k, r.temp, r.seed, r.stream + (shifts << 24))) return rc;
    if constexpr ((M & kPenalty) != 0)
        if (r.penalises())
            if (const int rc = gten_hip_decoder_set_penalty(dec, q, r.rep, r.freq, r.pres, pen_start, r.last_n)) return rc;
    return 0;
}

// ---- one sequence: generate<M> with r.shift_keep >= 0 (below 0: generate<M> itself).  `why` receives the text of a refusal.
template <unsigned M>
int generate_shifting(TinyLlama& model, std::vector<int32_t>& tokens, const int n_predict, const int eos, const Request& r, int max_ctx,
                      ShiftCounts* counts = nullptr, const char** why = nullptr)
{
    static_assert((M & kSampled) != 0, "the first id is drawn on the device");
    if (r.shift_keep < 0) return generate<M>(model, tokens, n_predict, eos, r, {}, nullptr, max_ctx);
    const int n_prompt = (int)tokens.size();
    if (const char* no = shift_refusal(r, n_prompt, max_ctx)) { if (why) *why = no; return -1; }
    if (n_prompt >= n_predict) return n_prompt;
    gten_hip_decoder* dec = model.decoder_handle();
    SlotRequests<M> slot(dec, 1);
    FsmHost fh(dec);
    if (slot.bind(0, r, n_prompt) != 0) return -1;
    {
        Tensor input{tokens.data(), {n_prompt}, kInt32};
        const Tensor logits = model.logits(input, 0);
        int32_t first = 0;
        Tensor id({1}, kInt32);
        draw_first<M>(dec, r, (const float*)logits.device_ptr(), logits.numel(), n_prompt, (int32_t*)id.device_ptr_mut(), nullptr, tokens.data(), &fh);
        GTEN_HIP_OK(gten_hip_memcpy_d2h(&first, id.device_ptr(), sizeof(first)));
        if (first == eos) return n_prompt;
        tokens.push_back(first);
    }
    if (slot.sample(0, r) != 0) return -1;
    std::vector<int32_t> view = tokens, out;               // what the model sees: ids [0, view.size()), rows [0, view.size() - 1)
    unsigned shifts = 0;
    int pen_start = r.start(n_prompt);
    while ((int)tokens.size() < n_predict) {
        ShiftPlan p;
        if (!shift_plan((int)view.size(), (int)view.size() - 1, max_ctx, r.shift_keep, r.shift_drop, &p)) return -1;
        if (p.due) {
            if (kv_shift_sets({&model}, {(int)view.size() - 1}, p.keep, {p.drop}, counts) != 0) return -1;
            view.resize((size_t)shift_ids(view.data(), (int)view.size(), p.keep, p.drop));
            pen_start = shift_phi(pen_start, p.keep, p.drop);
            if (rebind_shifted<M>(dec, 0, r, ++shifts, pen_start) != 0) return -1;
        }
        const int n_first = (int)view.size(), room = std::min(n_predict - (int)tokens.size(), max_ctx - n_first + 1);
        out.resize((size_t)room);
        const int got = model.decode_generate(view.data(), n_first, room, eos, out.data());
        tokens.insert(tokens.end(), out.begin(), out.begin() + got);
        view.insert(view.end(), out.begin(), out.begin() + got);
        if (got < room) break;                              // an eos
    }
    return slot.clear() ? -1 : (int)tokens.size();
}

// ---- a fixed batch: generate_batch<M> with a (keep, drop) pair for every sequence (keep < 0: generate_batch<M> itself).  A segment
// is one decode_generate over all sequences, each with the room its own window leaves; every live sequence ends it finished or with
// its window full, so all that are due shift together in one device call.
template <unsigned M>
int generate_batch_shifting(TinyLlamaBatch& batch, int max_ctx, const int32_t* prompts, const int32_t* n_prompt, int max_prompt, int max_tokens, int eos,
                            const Requests& reqs, int keep, int drop, int32_t* out, int32_t* n_total, ShiftCounts* counts = nullptr, const char** why = nullptr)
{
    static_assert((M & kSampled) != 0, "the first ids are drawn on the device");
    if (keep < 0) return generate_batch<M>(batch, max_ctx, prompts, n_prompt, max_prompt, max_tokens, eos, reqs, out, n_total);
    const int S = batch.n_seq();
    for (int q = 0; q < S; q++)
        if (n_prompt[q] <= 0 || n_prompt[q] > max_prompt || n_prompt[q] >= max_tokens) return -1;
    if (!reqs.ok(S, 0)) return -1;
    for (int q = 0; q < S; q++) {
        Request r = reqs[q];
        r.shift_keep = keep;
        r.shift_drop = drop;
        if (const char* no = shift_refusal(r, n_prompt[q], max_ctx)) { if (why) *why = no; return -1; }
    }
    gten_hip_decoder* dec = batch.decoder_handle();
    SlotRequests<M> slots(dec, S);
    FsmHost fh(dec);
    for (int q = 0; q < S; q++)
        if (const int rc = slots.bind(q, reqs[q], n_prompt[q])) return rc;
    std::vector<std::vector<int32_t>> view((size_t)S);
    std::vector<int> total((size_t)S), pen_start((size_t)S);
    std::vector<unsigned> shifts((size_t)S, 0);
    std::vector<char> live((size_t)S, 1);
    for (int q = 0; q < S; q++) {
        const int P = n_prompt[q];
        int32_t* row = out + (size_t)q * max_tokens;
        std::memcpy(row, prompts + (size_t)q * max_prompt, (size_t)P * sizeof(int32_t));
        const int32_t first = first_id<M>(batch, q, std::vector<int32_t>(row, row + P), reqs[q], nullptr, &fh);
        view[(size_t)q].assign(row, row + P);
        total[(size_t)q] = P;
        pen_start[(size_t)q] = reqs[q].start(P);
        if (first == eos) live[(size_t)q] = 0;
        else { row[P] = first; view[(size_t)q].push_back(first); total[(size_t)q] = P + 1; }
        if (total[(size_t)q] >= max_tokens) live[(size_t)q] = 0;
        if (const int rc = slots.sample(q, reqs[q])) return rc;
    }
    std::vector<int> n_first((size_t)S), room((size_t)S), n_out((size_t)S);
    std::vector<int32_t> gen;
    for (;;) {
        // the sequences that are due, in one device call
        std::vector<TinyLlama*> sets;
        std::vector<int> rows, drops, who;
        for (int q = 0; q < S; q++) {
            if (!live[(size_t)q]) continue;
            ShiftPlan p;
            if (!shift_plan((int)view[(size_t)q].size(), (int)view[(size_t)q].size() - 1, max_ctx, keep, drop, &p)) return -1;
            if (!p.due) continue;
            sets.push_back(&batch.seq(q));
            rows.push_back((int)view[(size_t)q].size() - 1);
            drops.push_back(p.drop);
            who.push_back(q);
        }
        if (const int rc = kv_shift_sets(sets, rows, keep, drops, counts)) return rc;
        for (size_t i = 0; i < who.size(); i++) {
            const int q = who[i];
            view[(size_t)q].resize((size_t)shift_ids(view[(size_t)q].data(), (int)view[(size_t)q].size(), keep, drops[i]));
            pen_start[(size_t)q] = shift_phi(pen_start[(size_t)q], keep, drops[i]);
            if (const int rc = rebind_shifted<M>(dec, q, reqs[q], ++shifts[(size_t)q], pen_start[(size_t)q])) return rc;
        }
        int max_new = 0, n_live = 0;
        for (int q = 0; q < S; q++) {
            // (a finished sequence is parked: it recomputes a row it has already computed, from the ids it was computed from)
            n_first[(size_t)q] = std::min((int)view[(size_t)q].size(), max_ctx);
            room[(size_t)q] = live[(size_t)q] ? std::min(max_tokens - total[(size_t)q], max_ctx - n_first[(size_t)q] + 1) : 0;
            max_new = std::max(max_new, room[(size_t)q]);
            n_live += live[(size_t)q] ? 1 : 0;
            batch.decode_set_tokens(q, view[(size_t)q].data(), 0, n_first[(size_t)q]);
        }
        if (n_live == 0) break;
        gen.resize((size_t)S * (size_t)max_new);
        batch.decode_generate(n_first.data(), max_new, eos, gen.data(), n_out.data(), room.data());
        for (int q = 0; q < S; q++) {
            if (!live[(size_t)q]) continue;
            const int take = std::min(n_out[(size_t)q], room[(size_t)q]);
            const int32_t* g = gen.data() + (size_t)q * (size_t)max_new;
            std::memcpy(out + (size_t)q * max_tokens + total[(size_t)q], g, (size_t)take * sizeof(int32_t));
            view[(size_t)q].insert(view[(size_t)q].end(), g, g + take);
            total[(size_t)q] += take;
            if (take < room[(size_t)q] || total[(size_t)q] >= max_tokens) live[(size_t)q] = 0;      // an eos, or its length
        }
    }
    for (int q = 0; q < S; q++) n_total[q] = total[(size_t)q];
    return slots.clear();
}

} // namespace gten
