// gten_decode_penalty.h -- repetition, frequency and presence penalties on the device (include/gten_hip_penalty.h);
// included by gten_decode.hip behind gten_decode_nucleus.h, whose step-end kernel this one extends by one stage in front.
//
// One workgroup of SMP_THREADS per row, as in every sampler kernel.  A penalised row first counts its window:
//   1. the counts c_i, dense u16, two per u32 word, in DYNAMIC LDS (pen_lds_bytes: 4 * ((n_vocab + 1) / 2) bytes -- 64 008 at 32003
//      ids, 131 072 at 65535): zeroed, then one LDS atomicAdd of 1 or 1 << 16 per window position.  A window has at most 65535
//      positions, so a half never carries into its neighbour.  Ids outside [0, n_vocab) are skipped -- parked slots and stale rows
//      exist.  Many equal ids hit one word and serialise; that is a window of a few thousand adds at the worst.
//   2. everything downstream is the code of §3.7 / §3.10 / §3.12 on the row y that smp_at<BIAS, true> forms wherever the row is read
//      (gten_decode_sample.h): p_i from (x_i, c_i), then the table.  The counts are integers and p_i is a function of (x_i, c_i):
//      nothing depends on the slot, the lane, the schedule or an order of additions.
// In the decoder the window is read from the sequence's own `tokens` row, which holds ids [0, n) when the step for context length n
// runs: no count table that a commit would have to keep in step, a slot that repeats its step derives the same counts, and the
// multi-step graphs need no host help.
#pragma once

struct PenParam {                // one sequence's penalty (gten_hip_decoder_set_penalty); 32 bytes
    float r, freq, pres;
    int start, last_n;           // window [max(start, last_n > 0 ? n - last_n : 0), n), clamped to [0, n]
    unsigned on;                 // 0: no penalty ((1, 0, 0), or never set) -- the sequence runs the cut rung's code
    unsigned pad[2];
};
static_assert(sizeof(PenParam) == 32, "PenParam is 32 bytes (include/gten_hip_penalty.h)");

static inline size_t pen_lds_bytes(int n_vocab) { return 4 * (((size_t)n_vocab + 1) / 2); }

// the counts of hist[0, len) into cnt (dynamic LDS, pen_lds_bytes(n_vocab)); the whole workgroup calls it
__device__ __forceinline__ void pen_count(unsigned* cnt, int n_vocab, const int32_t* hist, int len)
{
    const int words = (n_vocab + 1) >> 1;
    for (int i = threadIdx.x; i < words; i += SMP_THREADS) cnt[i] = 0u;
    __syncthreads();
    for (int i = threadIdx.x; i < len; i += SMP_THREADS) {
        const int id = hist[i];
        if ((unsigned)id < (unsigned)n_vocab) atomicAdd(&cnt[id >> 1], (id & 1) ? 0x10000u : 1u);
    }
    __syncthreads();
}

// One row's id: under the cut where one is on and the row samples, otherwise by smp_row; b null: no table.  PEN: from the penalised row.
template <bool PEN>
__device__ __forceinline__ int pen_draw(const float* __restrict__ x, const float* __restrict__ b, int n_vocab, int top_k, float temp, unsigned pos,
                                        unsigned stream, unsigned k0, unsigned k1, bool cut, float top_p, float tmin, CutInfo* __restrict__ info,
                                        SmpShared& sm, CutShared& cs, const PenRow& pr)
{
    if (cut && top_k > 0) {
        if (b) return smp_row_cut<true, PEN>(x, b, n_vocab, top_k, temp, pos, stream, k0, k1, top_p, tmin, info, sm, cs, pr);
        return smp_row_cut<false, PEN>(x, nullptr, n_vocab, top_k, temp, pos, stream, k0, k1, top_p, tmin, info, sm, cs, pr);
    }
    if (b) return smp_row<true, PEN>(x, b, n_vocab, top_k, temp, pos, stream, k0, k1, sm, pr);
    return smp_row<false, PEN>(x, nullptr, n_vocab, top_k, temp, pos, stream, k0, k1, sm, pr);
}

// k_dec_sample_cut for a decoder in which a sequence has set a penalty (pen0: [sequences]; cut0 null: nobody ever cut): a sequence
// whose penalty is on counts its window of its `tokens` row and draws -- greedy, top-k, under its cut, under its table -- from the
// penalised row; every other one runs exactly what k_dec_sample_cut runs.  The record is computed from the raw row x, as ever.  The
// choice is per workgroup, outside every pass.
__global__ __launch_bounds__(SMP_THREADS) void k_dec_sample_pen(const float* __restrict__ logits0, int n_vocab, int row_stride, const SampleParam* __restrict__ par0,
                                                               DecStep* step0, int32_t* __restrict__ result0, int result_stride,
                                                               int32_t* tokens0, int tok_stride, const float* __restrict__ bias0,
                                                               LpRecord* __restrict__ rec0, int rec_stride, const CutParam* __restrict__ cut0,
                                                               const PenParam* __restrict__ pen0)
{
    __shared__ SmpShared sm;
    __shared__ LpShared lps;
    __shared__ CutShared cs;
    const SampleParam p = par0[blockIdx.x];
    const PenParam pn = pen0[blockIdx.x];
    const bool cut = cut0 && cut0[blockIdx.x].on != 0u;
    const float top_p = cut ? cut0[blockIdx.x].top_p : 1.f, tmin = cut ? cut0[blockIdx.x].t : -INFINITY;
    DecStep* step = step0 + blockIdx.x;
    const int n = step->n;
    const unsigned pos = (unsigned)n;
    const float* x = logits0 + (size_t)blockIdx.x * row_stride;
    int32_t* tokens = tokens0 + (size_t)blockIdx.x * tok_stride;
    const bool biased = bias0 && p.table1 > 0 && (p.until == 0u || pos < p.until);
    const float* b = biased ? bias0 + (size_t)(p.table1 - 1) * (size_t)n_vocab : nullptr;
    int idx;
    if (pn.on != 0u) {
        unsigned* cnt = (unsigned*)g_smem;
        const int hi = min(max(n, 0), tok_stride);          // (the row has tok_stride ids: a step word outside the contract stays inside it)
        const int lo = min(max(max(pn.start, pn.last_n > 0 ? hi - pn.last_n : 0), 0), hi);
        pen_count(cnt, n_vocab, tokens + lo, hi - lo);
        idx = pen_draw<true>(x, b, n_vocab, p.top_k, p.temp, pos, p.stream, p.seed_lo, p.seed_hi, cut, top_p, tmin, nullptr, sm, cs, PenRow{cnt, pn.r, pn.freq, pn.pres});
    } else {
        idx = pen_draw<false>(x, b, n_vocab, p.top_k, p.temp, pos, p.stream, p.seed_lo, p.seed_hi, cut, top_p, tmin, nullptr, sm, cs, PenRow{});
    }
    if (rec0 && p.lp1 > 0u && pos < (unsigned)rec_stride) {
        LpRecord* r = rec0 + (size_t)blockIdx.x * (size_t)rec_stride + pos;
        smp_logprobs_row(x, n_vocab, min((int)p.lp1 - 1, LP_TOP), idx, LP_TOP, &r->lse, &r->logprob, r->top_id, r->top_logprob, sm, lps);
    }
    if (threadIdx.x == 0) dec_pick_commit(step, result0 + (size_t)blockIdx.x * result_stride, tokens, idx);
}

// gten_hip_sample_rows_pen: k_sample_rows_cut with row r's history hist[off[r], off[r + 1]) counted first where its penalty is on
__global__ __launch_bounds__(SMP_THREADS) void k_sample_rows_pen(const float* __restrict__ logits, int n_vocab, long long row_stride,
                                                                const float* __restrict__ bias, long long bias_stride,
                                                                const SampleRowParam* __restrict__ par, const CutParam* __restrict__ cut,
                                                                const PenParam* __restrict__ pen, const int32_t* __restrict__ hist,
                                                                const int32_t* __restrict__ off, unsigned seed_lo, unsigned seed_hi,
                                                                int32_t* __restrict__ out, CutInfo* __restrict__ info)
{
    __shared__ SmpShared sm;
    __shared__ CutShared cs;
    const SampleRowParam p = par[blockIdx.x];
    const CutParam c = cut[blockIdx.x];
    const PenParam pn = pen[blockIdx.x];
    const float* x = logits + (size_t)blockIdx.x * (size_t)row_stride;
    const float* b = bias ? bias + (size_t)blockIdx.x * (size_t)bias_stride : nullptr;
    CutInfo* inf = info ? info + blockIdx.x : nullptr;
    const bool cutting = p.top_k > 0 && (c.on != 0u || inf);
    int idx;
    if (pn.on != 0u) {
        unsigned* cnt = (unsigned*)g_smem;
        const int h0 = off[blockIdx.x];
        pen_count(cnt, n_vocab, hist + h0, off[blockIdx.x + 1] - h0);
        idx = pen_draw<true>(x, b, n_vocab, p.top_k, p.temp, p.pos, p.stream, seed_lo, seed_hi, cutting, c.top_p, c.t, inf, sm, cs, PenRow{cnt, pn.r, pn.freq, pn.pres});
    } else {
        idx = pen_draw<false>(x, b, n_vocab, p.top_k, p.temp, p.pos, p.stream, seed_lo, seed_hi, cutting, c.top_p, c.t, inf, sm, cs, PenRow{});
    }
    if (inf && !cutting && threadIdx.x == 0) { inf->Z = 0ull; inf->n_cand = 0; inf->n_nucleus = 0; inf->n_minp = 0; inf->n_keep = 0; }
    if (threadIdx.x == 0) out[blockIdx.x] = idx;
}

// gten_hip_penalize_rows: the row y the draw would be made from, written out -- the accessor itself, element by element
__global__ __launch_bounds__(SMP_THREADS) void k_penalize_rows(const float* __restrict__ logits, int n_vocab, long long row_stride,
                                                              const float* __restrict__ bias, long long bias_stride,
                                                              const PenParam* __restrict__ pen, const int32_t* __restrict__ hist,
                                                              const int32_t* __restrict__ off, float* __restrict__ y, long long y_stride)
{
    const PenParam pn = pen[blockIdx.x];
    const float* x = logits + (size_t)blockIdx.x * (size_t)row_stride;
    const float* b = bias ? bias + (size_t)blockIdx.x * (size_t)bias_stride : nullptr;
    float* yr = y + (size_t)blockIdx.x * (size_t)y_stride;
    if (pn.on != 0u) {
        unsigned* cnt = (unsigned*)g_smem;
        const int h0 = off[blockIdx.x];
        pen_count(cnt, n_vocab, hist + h0, off[blockIdx.x + 1] - h0);
        const PenRow pr{cnt, pn.r, pn.freq, pn.pres};
        for (int i = threadIdx.x; i < n_vocab; i += SMP_THREADS) yr[i] = b ? smp_at<true, true>(x, b, i, pr) : smp_at<false, true>(x, nullptr, i, pr);
    } else {
        for (int i = threadIdx.x; i < n_vocab; i += SMP_THREADS) yr[i] = b ? smp_at<true>(x, b, i) : smp_at<false>(x, nullptr, i);
    }
}
