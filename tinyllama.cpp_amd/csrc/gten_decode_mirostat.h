// gten_decode_mirostat.h -- Mirostat v2 on the device: the surprise of the generated text held at a target by a threshold mu that
// moves after every id (include/gten_hip_mirostat.h); included by gten_decode.hip behind gten_decode_fsm.h, whose
// step-end kernel this one extends by one stage.  The arithmetic is gten_miro_math.h's, shared with the host.
//
// One workgroup of SMP_THREADS per row y (the penalty first, then the table or the automaton's mask), as in every sampler kernel:
//   1. the candidates C, mx, a_j, q_j and Z exactly as smp_row_cut (gten_decode_nucleus.h) forms them -- integer masses, integer sum;
//   2. L = lg16(Z) - mu; T = the smallest mass with lg16(T) >= L, found once per row (miro_threshold: lg16 is monotone, so comparing
//      masses with T keeps the same set as comparing their logarithms with L); the kept set F = {the first of C} + {q_j >= T}, a
//      prefix of C;
//   3. one pass over C: Zk = sum of the kept masses, n_keep, and the draw of smp_row restricted to F;
//   4. s = lg16(Zk) - lg16(q_id), mu' = miro_update(mu, s).
// At most SMP_THREADS candidates: steps 1-3 run on the candidates compacted into LDS, one per thread (smp_row_cut's compaction); above,
// on the row -- the Z pass and the pass of step 3.  No float enters a decision except a_j and expf, which §3.12 already has.
// mu is kept per position like the automaton's state (gten_decode_fsm.h): a slot that repeats its step reads the same mu[n] and
// rewrites the same mu[n + 1]; the multi-step graphs need no host help; a sequence bound at `pos` never looks behind pos.
//
// The rung below sits at the scalar register limit (§3.15), and a row under Mirostat has eight more words of request than one without.
// So the request goes through LDS (MiroShared, written by thread 0 before the select's first barrier): what the routine needs behind the
// select -- temperature, noise counter, mu, tau, eta -- it reads from there into vector registers, and nothing of it lives in scalar
// registers across the select.  The row's facts come back the same way, for the thread that commits.
#pragma once

#include "gten_miro_math.h"

struct MiroParam {               // one sequence's binding (gten_hip_decoder_set_seq_mirostat); 16 bytes
    int tau_q, eta_q;            // Q16, formed on the host
    int pos;                     // the first position whose id is drawn under mu
    unsigned on;                 // 0: unbound -- the sequence runs the automaton rung's code
};
struct MiroRowParam {            // one row of gten_hip_sample_rows_miro; 16 bytes
    int mu, tau_q, eta_q;
    unsigned on;                 // 0: tau 0 -- the row draws by the routine below
};
struct MiroInfo {                // gten_hip_miro_info; 48 bytes
    unsigned long long Z, Zk, q_id;
    int32_t n_cand, n_keep, s, mu_next, pad[2];
};
static_assert(sizeof(MiroParam) == 16 && sizeof(MiroRowParam) == 16 && sizeof(MiroInfo) == 48, "include/gten_hip_mirostat.h: 16, 16 and 48 bytes");

struct MiroShared {
    // the request: thread 0 writes it before the row routine is called
    int mu, tau_q, eta_q;
    float temp;
    unsigned pos, stream, k0, k1;
    // the row's facts: thread 0 writes them at the end of the row routine, and reads them back itself
    MiroInfo out;
    // the decoder's commit: where thread 0 writes the next state and the next mu (null: not bound here), kept here across the draw
    int32_t *st_n, *mu_n;
};

__device__ __forceinline__ void miro_request(MiroShared& ms, int mu, int tau_q, int eta_q, float temp, unsigned pos, unsigned stream, unsigned k0, unsigned k1)
{
    if (threadIdx.x == 0) { ms.mu = mu; ms.tau_q = tau_q; ms.eta_q = eta_q; ms.temp = temp; ms.pos = pos; ms.stream = stream; ms.k0 = k0; ms.k1 = k1; }
}

// One sampling row (top_k >= 1) under Mirostat, its request in ms (miro_request; the select's barriers stand between that write and the
// reads here).  Every thread returns the id; afterwards thread 0 finds the row's facts in ms.out.
template <bool BIAS, bool PEN = false, bool FSM = false>
__device__ __forceinline__ int smp_row_miro(const float* __restrict__ x, const float* __restrict__ b, int n, int top_k, MiroShared& ms, SmpShared& sm,
                                            CutShared& cs, const PenRow& pen = PenRow{}, const FsmRow& fsm = FsmRow{})
{
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const SmpSelect sel = smp_select<BIAS, PEN, FSM>(x, b, n, top_k, sm, pen, fsm);
    const unsigned mask = sel.mask, prefix = sel.prefix, kmx = smp_key(sel.mx);
    const int ilim = sel.ilim, n_cand = min(top_k, n);
    const float mx = sel.mx;
    const float temp = ms.temp;
    const unsigned pos = ms.pos, stream = ms.stream, k0 = ms.k0, k1 = ms.k1;
    const int mu = ms.mu;
    unsigned long long Z = 0ull, zk = 0ull;
    unsigned cnt = 0u;
    float best = -INFINITY;
    int idx = 0x7fffffff;
    if (n_cand <= SMP_THREADS) {
        // one candidate per thread, compacted as smp_row_cut compacts them
        if (t == 0) cs.have = 0u;
        cs.cq[t] = 0ull;
        __syncthreads();
        for (int i = t; i < n; i += SMP_THREADS) {
            const float v = smp_at<BIAS, PEN, FSM>(x, b, i, pen, fsm);
            const unsigned key = smp_key(v), km = key & mask;
            if (km > prefix || (km == prefix && i <= ilim)) {
                const unsigned slot = atomicAdd(&cs.have, 1u);
                if (slot < (unsigned)SMP_THREADS) {                     // (the bound keeps a row outside the contract -- NaN -- inside the arrays)
                    cs.ckey[slot] = key; cs.cidx[slot] = i;
                    cs.cq[slot] = cut_mass(cut_score(v, mx, temp));
                }
            }
        }
        __syncthreads();
        const int have = (int)min(cs.have, (unsigned)n_cand);
        const bool mine = t < have;
        const unsigned key = mine ? cs.ckey[t] : 0u;
        const int ci = mine ? cs.cidx[t] : 0x7fffffff;
        const unsigned long long q = cs.cq[t];
        // (-0 and +0 share a key and a score of equal value: the key gives the score back)
        const float a = mine ? cut_score(cut_unkey(key), mx, temp) : -INFINITY;
        unsigned long long z = q;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o, 64);
        if (lane == 0) cs.wz[wid] = z;
        __syncthreads();
        for (int w = 0; w < SMP_WAVES; w++) Z += cs.wz[w];
        // the first of C: the lowest index among the maxima (the reduction's barriers stand between the reads of wz above and
        // the writes below)
        const int first = smp_block_argmax(mine && key == kmx ? 0.f : -INFINITY, ci, sm);
        const unsigned long long T = miro_threshold(miro_lg16(Z) - mu, CUT_MASS_BITS);
        if (mine && (ci == first || q >= T)) { zk = q; cnt = 1u; best = a + smp_gumbel((unsigned)ci, pos, stream, k0, k1); idx = ci; }
    } else {
        // the Z pass over C, and the first of C
        int fi = 0x7fffffff;
        unsigned long long z = 0ull;
        for (int i = t; i < n; i += SMP_THREADS) {
            const float v = smp_at<BIAS, PEN, FSM>(x, b, i, pen, fsm);
            const unsigned key = smp_key(v), km = key & mask;
            if (km > prefix || (km == prefix && i <= ilim)) {
                z += cut_mass(cut_score(v, mx, temp));
                if (key == kmx && i < fi) fi = i;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o, 64);
        if (lane == 0) cs.wz[wid] = z;
        __syncthreads();
        for (int w = 0; w < SMP_WAVES; w++) Z += cs.wz[w];
        const int first = smp_block_argmax(fi != 0x7fffffff ? 0.f : -INFINITY, fi, sm);
        const unsigned long long T = miro_threshold(miro_lg16(Z) - mu, CUT_MASS_BITS);
        // Zk, n_keep and the draw over F
        for (int i = t; i < n; i += SMP_THREADS) {
            const float v = smp_at<BIAS, PEN, FSM>(x, b, i, pen, fsm);
            const unsigned km = smp_key(v) & mask;
            if (km > prefix || (km == prefix && i <= ilim)) {
                const float a = cut_score(v, mx, temp);
                const unsigned long long q = cut_mass(a);
                if (i == first || q >= T) {
                    zk += q; cnt++;
                    const float s = a + smp_gumbel((unsigned)i, pos, stream, k0, k1);
                    if (s > best || (s == best && i < idx)) { best = s; idx = i; }
                }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { zk += __shfl_xor(zk, o, 64); cnt += __shfl_xor(cnt, o, 64); }
    if (lane == 0) { cs.wz[wid] = zk; cs.wc[wid] = cnt; }
    idx = smp_block_argmax(best, idx, sm);         // (its barriers order wz and wc)
    if (t == 0) {
        unsigned long long Zk = 0ull;
        unsigned n_keep = 0u;
        for (int w = 0; w < SMP_WAVES; w++) { Zk += cs.wz[w]; n_keep += cs.wc[w]; }
        // the winner's mass, by the expression that formed it (a member of F other than the first has q >= 1, the first has 2^36)
        const unsigned long long q_id = (unsigned)idx < (unsigned)n ? cut_mass(cut_score(smp_at<BIAS, PEN, FSM>(x, b, idx, pen, fsm), mx, temp)) : 0ull;
        const int s = miro_lg16(Zk) - miro_lg16(q_id);
        ms.out.Z = Z; ms.out.Zk = Zk; ms.out.q_id = q_id;
        ms.out.n_cand = n_cand; ms.out.n_keep = (int)n_keep; ms.out.s = s; ms.out.mu_next = miro_update(mu, s, ms.tau_q, ms.eta_q);
        ms.out.pad[0] = 0; ms.out.pad[1] = 0;
    }
    return idx;
}

// smp_row_miro from the row the rung below would draw from: masked (fr.next not null; a bound sequence has no table), under a table
// (b not null), or neither
template <bool PEN>
__device__ __forceinline__ int miro_draw(const float* __restrict__ x, const float* __restrict__ b, int n_vocab, int top_k, MiroShared& ms, SmpShared& sm,
                                         CutShared& cs, const PenRow& pr, const FsmRow& fr)
{
    if (fr.next) return smp_row_miro<false, PEN, true>(x, nullptr, n_vocab, top_k, ms, sm, cs, pr, fr);
    if (b) return smp_row_miro<true, PEN>(x, b, n_vocab, top_k, ms, sm, cs, pr);
    return smp_row_miro<false, PEN>(x, nullptr, n_vocab, top_k, ms, sm, cs, pr);
}

// gten_hip_sample_rows_miro: k_sample_rows_fsm without a cut, with an optional bias row (the host refuses a bias beside a state), row r
// under Mirostat where mr[r].on; a greedy row and a row with tau 0 draw by the routine below and report zeros and mu_next = mu
__global__ __launch_bounds__(SMP_THREADS) void k_sample_rows_miro(const float* __restrict__ logits, int n_vocab, long long row_stride,
                                                                 const float* __restrict__ bias, long long bias_stride,
                                                                 const SampleRowParam* __restrict__ par, const PenParam* __restrict__ pen,
                                                                 const int32_t* __restrict__ hist, const int32_t* __restrict__ off,
                                                                 const uint16_t* __restrict__ next, const uint8_t* __restrict__ flags, int n_states,
                                                                 const int32_t* __restrict__ st, const MiroRowParam* __restrict__ mr,
                                                                 unsigned seed_lo, unsigned seed_hi, int32_t* __restrict__ out,
                                                                 int32_t* __restrict__ nxt, MiroInfo* __restrict__ info)
{
    __shared__ SmpShared sm;
    __shared__ CutShared cs;
    __shared__ MiroShared ms;
    const SampleRowParam p = par[blockIdx.x];
    const PenParam pn = pen[blockIdx.x];
    const float* x = logits + (size_t)blockIdx.x * (size_t)row_stride;
    const float* b = bias ? bias + (size_t)blockIdx.x * (size_t)bias_stride : nullptr;
    const int s = fsm_live(st[blockIdx.x], n_states, flags);
    const FsmRow fr{s >= 0 ? next + (size_t)s * (size_t)n_vocab : nullptr};
    const bool miro = mr[blockIdx.x].on != 0u && p.top_k > 0;
    PenRow pr{};
    if (pn.on != 0u) {
        unsigned* cnt = (unsigned*)g_smem;
        const int h0 = off[blockIdx.x];
        pen_count(cnt, n_vocab, hist + h0, off[blockIdx.x + 1] - h0);
        pr = PenRow{cnt, pn.r, pn.freq, pn.pres};
    }
    int idx;
    if (miro) {
        const MiroRowParam m = mr[blockIdx.x];
        miro_request(ms, m.mu, m.tau_q, m.eta_q, p.temp, p.pos, p.stream, seed_lo, seed_hi);
        if (pn.on != 0u) idx = miro_draw<true>(x, b, n_vocab, p.top_k, ms, sm, cs, pr, fr);
        else idx = miro_draw<false>(x, b, n_vocab, p.top_k, ms, sm, cs, PenRow{}, fr);
    } else if (fr.next) {
        if (pn.on != 0u) idx = fsm_draw<true>(x, n_vocab, p.top_k, p.temp, p.pos, p.stream, seed_lo, seed_hi, false, 1.f, -INFINITY, nullptr, sm, cs, pr, fr);
        else idx = fsm_draw<false>(x, n_vocab, p.top_k, p.temp, p.pos, p.stream, seed_lo, seed_hi, false, 1.f, -INFINITY, nullptr, sm, cs, PenRow{}, fr);
    } else if (pn.on != 0u) {
        idx = pen_draw<true>(x, b, n_vocab, p.top_k, p.temp, p.pos, p.stream, seed_lo, seed_hi, false, 1.f, -INFINITY, nullptr, sm, cs, pr);
    } else {
        idx = pen_draw<false>(x, b, n_vocab, p.top_k, p.temp, p.pos, p.stream, seed_lo, seed_hi, false, 1.f, -INFINITY, nullptr, sm, cs, PenRow{});
    }
    if (threadIdx.x == 0) {
        if (info) {
            MiroInfo* inf = info + blockIdx.x;
            if (miro) *inf = ms.out;
            else { *inf = MiroInfo{}; inf->mu_next = mr[blockIdx.x].mu; }
        }
        out[blockIdx.x] = idx;
        if (nxt) {
            const int s_here = st[blockIdx.x];
            const bool in_pool = (unsigned)s_here < (unsigned)n_states;
            nxt[blockIdx.x] = (fr.next && (unsigned)idx < (unsigned)n_vocab) ? (int)fr.next[idx] : (in_pool ? s_here : -1);
        }
    }
}

// k_dec_sample_fsm for a decoder in which a sequence has been bound to Mirostat (miro0: [sequences]; mu0: [sequences][rec_stride], laid
// out like state0; fsm0 / pen0 / cut0 null: nobody ever used them).  A sequence bound at or before this position that samples draws by
// smp_row_miro from the row the rung below would draw from -- penalised, then under its table or its automaton's mask -- and commits
// mu[n + 1]; every other one, a bound one that is greedy included, runs exactly what k_dec_sample_fsm runs and leaves the mu row alone
// (a greedy step may end in k_dec_argmax, which knows no mu: so no greedy step writes one).  The choice is per workgroup, outside every
// pass.  The record is computed from the raw row x, as ever.
__global__ __launch_bounds__(SMP_THREADS) void k_dec_sample_miro(const float* __restrict__ logits0, int n_vocab, int row_stride, const SampleParam* __restrict__ par0,
                                                                DecStep* step0, int32_t* __restrict__ result0, int result_stride,
                                                                int32_t* tokens0, int tok_stride, const float* __restrict__ bias0,
                                                                LpRecord* __restrict__ rec0, int rec_stride, const CutParam* __restrict__ cut0,
                                                                const PenParam* __restrict__ pen0, const uint16_t* __restrict__ next0,
                                                                const uint8_t* __restrict__ flags0, int n_states, const FsmParam* __restrict__ fsm0,
                                                                int32_t* state0, const MiroParam* __restrict__ miro0, int32_t* mu0)
{
    __shared__ SmpShared sm;
    __shared__ LpShared lps;
    __shared__ CutShared cs;
    __shared__ MiroShared ms;
    const SampleParam p = par0[blockIdx.x];
    const bool pen_on = pen0 && pen0[blockIdx.x].on != 0u;
    DecStep* step = step0 + blockIdx.x;
    const int n = step->n;
    const unsigned pos = (unsigned)n;
    const float* x = logits0 + (size_t)blockIdx.x * row_stride;
    int32_t* tokens = tokens0 + (size_t)blockIdx.x * tok_stride;
    // (both rows have rec_stride entries: a step word outside the contract touches neither entry n nor entry n + 1.  What outlives
    //  the draw is kept smaller than in the rung below: st_n / mu_n -- null for "not bound here" -- wait in LDS for the committing thread)
    const bool in_row = n >= 0 && n + 1 < rec_stride;
    const bool bound = fsm0 && fsm0[blockIdx.x].on != 0u && n >= fsm0[blockIdx.x].pos && in_row;
    int32_t* st_n = bound ? state0 + (size_t)blockIdx.x * (size_t)rec_stride + n : nullptr;
    const int s = fsm_live(bound ? st_n[0] : -1, n_states, flags0);
    const uint16_t* row = s >= 0 ? next0 + (size_t)s * (size_t)n_vocab : nullptr;
    const bool miro = miro0[blockIdx.x].on != 0u && n >= miro0[blockIdx.x].pos && in_row && p.top_k > 0;
    int32_t* mu_n = miro ? mu0 + (size_t)blockIdx.x * (size_t)rec_stride + n : nullptr;
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
    if (threadIdx.x == 0) { ms.st_n = st_n; ms.mu_n = mu_n; }
    int idx;
    if (miro) {
        // (a sequence bound here has no cut: the setters refuse the pair)
        miro_request(ms, mu_n[0], miro0[blockIdx.x].tau_q, miro0[blockIdx.x].eta_q, p.temp, pos, p.stream, p.seed_lo, p.seed_hi);
        if (pen_on) idx = miro_draw<true>(x, b, n_vocab, p.top_k, ms, sm, cs, pr, FsmRow{row});
        else idx = miro_draw<false>(x, b, n_vocab, p.top_k, ms, sm, cs, PenRow{}, FsmRow{row});
    } else {
        const bool cut = cut0 && cut0[blockIdx.x].on != 0u;
        const float top_p = cut ? cut0[blockIdx.x].top_p : 1.f, tmin = cut ? cut0[blockIdx.x].t : -INFINITY;
        if (row) {
            const FsmRow fr{row};
            if (pen_on) idx = fsm_draw<true>(x, n_vocab, p.top_k, p.temp, pos, p.stream, p.seed_lo, p.seed_hi, cut, top_p, tmin, nullptr, sm, cs, pr, fr);
            else idx = fsm_draw<false>(x, n_vocab, p.top_k, p.temp, pos, p.stream, p.seed_lo, p.seed_hi, cut, top_p, tmin, nullptr, sm, cs, PenRow{}, fr);
        } else if (pen_on) {
            idx = pen_draw<true>(x, b, n_vocab, p.top_k, p.temp, pos, p.stream, p.seed_lo, p.seed_hi, cut, top_p, tmin, nullptr, sm, cs, pr);
        } else {
            idx = pen_draw<false>(x, b, n_vocab, p.top_k, p.temp, pos, p.stream, p.seed_lo, p.seed_hi, cut, top_p, tmin, nullptr, sm, cs, PenRow{});
        }
    }
    if (rec) smp_logprobs_row(x, n_vocab, min((int)p.lp1 - 1, LP_TOP), idx, LP_TOP, &rec->lse, &rec->logprob, rec->top_id, rec->top_logprob, sm, lps);
    if (threadIdx.x == 0) {
        // (before the commit, which bumps step->n)
        // (a pointer that comes out of LDS is generic to the compiler: said to be global again, the accesses stay global_load / global_store)
        typedef __attribute__((address_space(1))) int32_t* g_i32p;
        const g_i32p st_c = (g_i32p)ms.st_n, mu_c = (g_i32p)ms.mu_n;
        if (st_c) st_c[1] = (row && (unsigned)idx < (unsigned)n_vocab) ? (int)row[idx] : st_c[0];
        if (mu_c) mu_c[1] = ms.out.mu_next;
        dec_pick_commit(step, result0 + (size_t)blockIdx.x * result_stride, tokens, idx);
    }
}
