// gten_decode_fsm.h -- token automata on the device: stop sequences and masked grammars (include/gten_hip_fsm.h);
// included by gten_decode.hip behind gten_decode_penalty.h, whose step-end kernel this one extends by one stage.
//
// One workgroup of SMP_THREADS per row, as in every sampler kernel.  A bound sequence reads s = state[n] of its own state row; where
// s is a live (non-final) state of the pool, the row the draw is made from is masked by the state's row of `next` -- smp_at<.., FSM>
// (gten_decode_sample.h) takes one u16 load per element it reads, the row (64 KB at 32003 ids) is re-read by the select's passes from
// L2 -- and the committing thread writes state[n + 1] = next[s][id].  Everything downstream of the accessor is the code of §3.7 /
// §3.12 / §3.14.  The choice between masked and unmasked code is made per workgroup, outside every pass: an unbound sequence, or a
// final one, runs the penalty rung's code.
// The state is kept per position, not as one word per sequence, so it is a function of (row, n) as the penalty's counts are: a slot
// that repeats its step (DecStep::stop) reads the same state[n] and rewrites the same state[n + 1]; the multi-step graphs need no
// host help; a sequence bound at `pos` never looks behind pos.
#pragma once

struct FsmParam {                // one sequence's binding (gten_hip_decoder_set_seq_fsm); 32 bytes
    int state;                   // the state at `pos` (the setter also writes it to the state row; kept here for fsm_info)
    int pos;                     // the first position whose id is chosen under the automaton
    unsigned on;                 // 0: unbound -- the sequence runs the penalty rung's code
    unsigned pad[5];
};
static_assert(sizeof(FsmParam) == 32, "FsmParam is 32 bytes (include/gten_hip_fsm.h)");
static_assert(FSM_DEAD == GTEN_HIP_FSM_DEAD, "gten_decode_sample.h and include/gten_hip_fsm.h disagree");

// the live state a row is masked by, or -1: `s` is unbound (-1), outside the pool (a stale row, a DEAD entry) or final
__device__ __forceinline__ int fsm_live(int s, int n_states, const uint8_t* __restrict__ flags)
{
    if ((unsigned)s >= (unsigned)n_states) return -1;
    return (flags[s] & GTEN_HIP_FSM_FINAL) ? -1 : s;
}

// pen_draw (gten_decode_penalty.h) from the row masked by fr: no table (a bound sequence has none)
template <bool PEN>
__device__ __forceinline__ int fsm_draw(const float* __restrict__ x, int n_vocab, int top_k, float temp, unsigned pos, unsigned stream, unsigned k0,
                                        unsigned k1, bool cut, float top_p, float tmin, CutInfo* __restrict__ info, SmpShared& sm, CutShared& cs,
                                        const PenRow& pr, const FsmRow& fr)
{
    if (cut && top_k > 0) return smp_row_cut<false, PEN, true>(x, nullptr, n_vocab, top_k, temp, pos, stream, k0, k1, top_p, tmin, info, sm, cs, pr, fr);
    return smp_row<false, PEN, true>(x, nullptr, n_vocab, top_k, temp, pos, stream, k0, k1, sm, pr, fr);
}

// k_dec_sample_pen for a decoder in which a sequence has been bound to an automaton (fsm0: [sequences]; pen0 / cut0 null: nobody ever
// penalised / cut; state0: [sequences][rec_stride], the records' stride: both rows have max_ctx + 2 entries).  A sequence bound at or before this position whose state is live draws from
// the masked row and commits its next state; every other one runs exactly what k_dec_sample_pen runs (a final one carries its state
// on).  The record is computed from the raw row x, as ever.
__global__ __launch_bounds__(SMP_THREADS) void k_dec_sample_fsm(const float* __restrict__ logits0, int n_vocab, int row_stride, const SampleParam* __restrict__ par0,
                                                               DecStep* step0, int32_t* __restrict__ result0, int result_stride,
                                                               int32_t* tokens0, int tok_stride, const float* __restrict__ bias0,
                                                               LpRecord* __restrict__ rec0, int rec_stride, const CutParam* __restrict__ cut0,
                                                               const PenParam* __restrict__ pen0, const uint16_t* __restrict__ next0,
                                                               const uint8_t* __restrict__ flags0, int n_states, const FsmParam* __restrict__ fsm0,
                                                               int32_t* state0)
{
    __shared__ SmpShared sm;
    __shared__ LpShared lps;
    __shared__ CutShared cs;
    const SampleParam p = par0[blockIdx.x];
    const FsmParam fp = fsm0[blockIdx.x];
    const bool pen_on = pen0 && pen0[blockIdx.x].on != 0u;
    const bool cut = cut0 && cut0[blockIdx.x].on != 0u;
    const float top_p = cut ? cut0[blockIdx.x].top_p : 1.f, tmin = cut ? cut0[blockIdx.x].t : -INFINITY;
    DecStep* step = step0 + blockIdx.x;
    const int n = step->n;
    const unsigned pos = (unsigned)n;
    const float* x = logits0 + (size_t)blockIdx.x * row_stride;
    int32_t* tokens = tokens0 + (size_t)blockIdx.x * tok_stride;
    // (the state row has rec_stride entries: a step word outside the contract touches neither state[n] nor state[n + 1].  What
    //  outlives the draw is kept small -- the kernel sits at the scalar register limit: st_n is null for "not bound here", row null
    //  for "not masked", and neither the pool's base nor the flags are needed behind this point)
    const bool bound = fp.on != 0u && n >= fp.pos && n >= 0 && n + 1 < rec_stride;
    int32_t* st_n = bound ? state0 + (size_t)blockIdx.x * (size_t)rec_stride + n : nullptr;
    const int s_here = bound ? st_n[0] : -1;
    const int s = fsm_live(s_here, n_states, flags0);
    const uint16_t* row = s >= 0 ? next0 + (size_t)s * (size_t)n_vocab : nullptr;
    LpRecord* rec = (rec0 && p.lp1 > 0u && pos < (unsigned)rec_stride) ? rec0 + (size_t)blockIdx.x * (size_t)rec_stride + pos : nullptr;
    const bool biased = bias0 && p.table1 > 0 && (p.until == 0u || pos < p.until);
    const float* b = biased ? bias0 + (size_t)(p.table1 - 1) * (size_t)n_vocab : nullptr;
    PenRow pr{};
    if (pen_on) {
        const PenParam pn = pen0[blockIdx.x];
        unsigned* cnt = (unsigned*)g_smem;
        const int hi = min(max(n, 0), tok_stride);
        const int lo = min(max(max(pn.start, pn.last_n > 0 ? hi - pn.last_n : 0), 0), hi);
        pen_count(cnt, n_vocab, tokens + lo, hi - lo);
        pr = PenRow{cnt, pn.r, pn.freq, pn.pres};
    }
    int idx;
    if (row) {
        const FsmRow fr{row};
        if (pen_on) idx = fsm_draw<true>(x, n_vocab, p.top_k, p.temp, pos, p.stream, p.seed_lo, p.seed_hi, cut, top_p, tmin, nullptr, sm, cs, pr, fr);
        else idx = fsm_draw<false>(x, n_vocab, p.top_k, p.temp, pos, p.stream, p.seed_lo, p.seed_hi, cut, top_p, tmin, nullptr, sm, cs, PenRow{}, fr);
    } else if (pen_on) {
        idx = pen_draw<true>(x, b, n_vocab, p.top_k, p.temp, pos, p.stream, p.seed_lo, p.seed_hi, cut, top_p, tmin, nullptr, sm, cs, pr);
    } else {
        idx = pen_draw<false>(x, b, n_vocab, p.top_k, p.temp, pos, p.stream, p.seed_lo, p.seed_hi, cut, top_p, tmin, nullptr, sm, cs, PenRow{});
    }
    if (rec) smp_logprobs_row(x, n_vocab, min((int)p.lp1 - 1, LP_TOP), idx, LP_TOP, &rec->lse, &rec->logprob, rec->top_id, rec->top_logprob, sm, lps);
    if (threadIdx.x == 0) {
        // (before the commit, which bumps step->n; a state that is not live -- final, stale -- is carried on as it is: read again)
        if (st_n) st_n[1] = (row && (unsigned)idx < (unsigned)n_vocab) ? (int)row[idx] : st_n[0];
        dec_pick_commit(step, result0 + (size_t)blockIdx.x * result_stride, tokens, idx);
    }
}

// gten_hip_sample_rows_fsm: k_sample_rows_pen without a table, row r in state st[r] of the pool; nxt[r] (nxt may be null) = next[s][id],
// s for a final row, -1 for one outside the pool
__global__ __launch_bounds__(SMP_THREADS) void k_sample_rows_fsm(const float* __restrict__ logits, int n_vocab, long long row_stride,
                                                                const SampleRowParam* __restrict__ par, const CutParam* __restrict__ cut,
                                                                const PenParam* __restrict__ pen, const int32_t* __restrict__ hist,
                                                                const int32_t* __restrict__ off, const uint16_t* __restrict__ next,
                                                                const uint8_t* __restrict__ flags, int n_states, const int32_t* __restrict__ st,
                                                                unsigned seed_lo, unsigned seed_hi, int32_t* __restrict__ out,
                                                                int32_t* __restrict__ nxt, CutInfo* __restrict__ info)
{
    __shared__ SmpShared sm;
    __shared__ CutShared cs;
    const SampleRowParam p = par[blockIdx.x];
    const CutParam c = cut[blockIdx.x];
    const PenParam pn = pen[blockIdx.x];
    const float* x = logits + (size_t)blockIdx.x * (size_t)row_stride;
    CutInfo* inf = info ? info + blockIdx.x : nullptr;
    const bool cutting = p.top_k > 0 && (c.on != 0u || inf);
    const int s_here = st[blockIdx.x];
    const int s = fsm_live(s_here, n_states, flags);
    PenRow pr{};
    if (pn.on != 0u) {
        unsigned* cnt = (unsigned*)g_smem;
        const int h0 = off[blockIdx.x];
        pen_count(cnt, n_vocab, hist + h0, off[blockIdx.x + 1] - h0);
        pr = PenRow{cnt, pn.r, pn.freq, pn.pres};
    }
    int idx;
    if (s >= 0) {
        const FsmRow fr{next + (size_t)s * (size_t)n_vocab};
        if (pn.on != 0u) idx = fsm_draw<true>(x, n_vocab, p.top_k, p.temp, p.pos, p.stream, seed_lo, seed_hi, cutting, c.top_p, c.t, inf, sm, cs, pr, fr);
        else idx = fsm_draw<false>(x, n_vocab, p.top_k, p.temp, p.pos, p.stream, seed_lo, seed_hi, cutting, c.top_p, c.t, inf, sm, cs, PenRow{}, fr);
    } else if (pn.on != 0u) {
        idx = pen_draw<true>(x, nullptr, n_vocab, p.top_k, p.temp, p.pos, p.stream, seed_lo, seed_hi, cutting, c.top_p, c.t, inf, sm, cs, pr);
    } else {
        idx = pen_draw<false>(x, nullptr, n_vocab, p.top_k, p.temp, p.pos, p.stream, seed_lo, seed_hi, cutting, c.top_p, c.t, inf, sm, cs, PenRow{});
    }
    if (inf && !cutting && threadIdx.x == 0) { inf->Z = 0ull; inf->n_cand = 0; inf->n_nucleus = 0; inf->n_minp = 0; inf->n_keep = 0; }
    if (threadIdx.x == 0) {
        out[blockIdx.x] = idx;
        if (nxt) {
            const bool in_pool = (unsigned)s_here < (unsigned)n_states;
            nxt[blockIdx.x] = (s >= 0 && (unsigned)idx < (unsigned)n_vocab) ? (int)next[(size_t)s * (size_t)n_vocab + (size_t)idx] : (in_pool ? s_here : -1);
        }
    }
}

// gten_hip_mask_rows_fsm: the row y the draw would be made from, written out -- the accessor itself, element by element
__global__ __launch_bounds__(SMP_THREADS) void k_mask_rows_fsm(const float* __restrict__ logits, int n_vocab, long long row_stride,
                                                              const PenParam* __restrict__ pen, const int32_t* __restrict__ hist,
                                                              const int32_t* __restrict__ off, const uint16_t* __restrict__ next,
                                                              const uint8_t* __restrict__ flags, int n_states, const int32_t* __restrict__ st,
                                                              float* __restrict__ y, long long y_stride)
{
    const PenParam pn = pen[blockIdx.x];
    const float* x = logits + (size_t)blockIdx.x * (size_t)row_stride;
    float* yr = y + (size_t)blockIdx.x * (size_t)y_stride;
    const int s = fsm_live(st[blockIdx.x], n_states, flags);
    PenRow pr{};
    if (pn.on != 0u) {
        unsigned* cnt = (unsigned*)g_smem;
        const int h0 = off[blockIdx.x];
        pen_count(cnt, n_vocab, hist + h0, off[blockIdx.x + 1] - h0);
        pr = PenRow{cnt, pn.r, pn.freq, pn.pres};
    }
    if (s >= 0) {
        const FsmRow fr{next + (size_t)s * (size_t)n_vocab};
        if (pn.on != 0u) for (int i = threadIdx.x; i < n_vocab; i += SMP_THREADS) yr[i] = smp_at<false, true, true>(x, nullptr, i, pr, fr);
        else for (int i = threadIdx.x; i < n_vocab; i += SMP_THREADS) yr[i] = smp_at<false, false, true>(x, nullptr, i, pr, fr);
    } else {
        if (pn.on != 0u) for (int i = threadIdx.x; i < n_vocab; i += SMP_THREADS) yr[i] = smp_at<false, true>(x, nullptr, i, pr);
        else for (int i = threadIdx.x; i < n_vocab; i += SMP_THREADS) yr[i] = smp_at<false>(x, nullptr, i);
    }
}
