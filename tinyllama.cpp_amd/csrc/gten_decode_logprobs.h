// gten_decode_logprobs.h -- the log-prob of a step's committed id and the top-N alternatives of its logits row, on the device
// (include/gten_hip_logprobs.h); included by gten_decode.hip behind gten_decode_sample.h, whose workgroup shape,
// key order and histogram helpers it uses.
//
// One workgroup of SMP_THREADS per RAW logits row x (no bias table, temperature 1, the whole vocabulary):
//   1. lse = max x + log(sum exp(x - max x)): each thread walks its elements in ascending index order with a running
//      (maximum, sum), the states merge across the wave by __shfl_xor and across the waves through LDS;
//   2. the n_top largest keys smp_key(x_j), ties at the n_top-th value to the lower index: the radix select of smp_row
//      (with the second select on the indices where several values equal the n_top-th);
//   3. the winners (at most LP_TOP) are compacted into LDS and each counts how many of the others precede it under
//      (key descending, index ascending): its place in the list;
//   4. the first LP_TOP threads write the entries, thread 0 lse and the committed id's log-prob.
// Steps 2 and 3 are integer facts about the row; x_j - lse is one f32 subtraction wherever it is formed, so the entry of an id
// equals the log-prob of the same id bit for bit.  Both kernels below call the one routine: a record of the decoder equals
// gten_hip_row_top_logprobs on the same row.
#pragma once

#define LP_TOP 20                // GTEN_HIP_LOGPROBS_TOP

// one position's record in the decoder's buffer: [n_seq][max_ctx + 2] of these, indexed by n like `result`; 168 bytes.
// Entries [min(n_top, n_vocab), LP_TOP) are id -1, logprob 0.
struct LpRecord {
    float lse;
    float logprob;               // x[id] - lse, id = result[n]
    int32_t top_id[LP_TOP];
    float top_logprob[LP_TOP];
};
static_assert(sizeof(LpRecord) == 168, "LpRecord is 168 bytes (include/gten_hip_logprobs.h)");
static_assert(sizeof(SampleParam) == 32, "SampleParam is 32 bytes: the log-prob request took its last pad word");

struct LpShared {
    float wm[SMP_WAVES], ws[SMP_WAVES];
    unsigned key[LP_TOP];
    int idx[LP_TOP];
    unsigned count;
};

__device__ __forceinline__ float lp_exp_le0(float d) { return __builtin_amdgcn_exp2f(d * 1.4426950408889634f); }   // d <= 0

// (m, s) += (om, os); an empty state (s == 0, m == -inf) is skipped, not formed as 0 * exp(-inf + inf)
__device__ __forceinline__ void lp_merge_ms(float& m, float& s, float om, float os)
{
    const float mn = fmaxf(m, om);
    const float sa = s == 0.f ? 0.f : s * lp_exp_le0(m - mn);
    const float sb = os == 0.f ? 0.f : os * lp_exp_le0(om - mn);
    m = mn;
    s = sa + sb;
}

// The record of one row.  id: the committed id (outside [0, n): no chosen id, log-prob 0).  n_slots entries are written to
// top_id / top_lp (n_top <= n_slots <= LP_TOP), the ones from min(n_top, n) on as -1 / 0; lse_out may be null.  Every thread of
// the workgroup calls it; `sm` may hold anything.
__device__ __forceinline__ void smp_logprobs_row(const float* __restrict__ x, int n, int n_top, int id, int n_slots, float* __restrict__ lse_out,
                                                 float* __restrict__ logprob_out, int32_t* __restrict__ top_id, float* __restrict__ top_lp,
                                                 SmpShared& sm, LpShared& lps)
{
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    // 1. log-sum-exp
    float m = -INFINITY, s = 0.f;
    for (int i = t; i < n; i += SMP_THREADS) {
        const float v = x[i];
        const float mn = fmaxf(m, v);
        s = (s == 0.f ? 0.f : s * lp_exp_le0(m - mn)) + lp_exp_le0(v - mn);
        m = mn;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lp_merge_ms(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
    __syncthreads();                               // (whoever used sm / lps before is done with them)
    if (lane == 0) { lps.wm[wid] = m; lps.ws[wid] = s; }
    if (t == 0) lps.count = 0u;
    __syncthreads();
    m = lps.wm[0]; s = lps.ws[0];
    for (int w = 1; w < SMP_WAVES; w++) lp_merge_ms(m, s, lps.wm[w], lps.ws[w]);
    const float lse = m + logf(s);                 // the same operands in the same order on every thread
    // 2. the threshold of the top n_top: (key & mask) > prefix, or == prefix with index <= ilim
    unsigned mask = 0u, prefix = 0u, kk = (unsigned)min(n_top, n);
    const int n_win = (int)kk;
    int ilim = 0x7fffffff;
    if (n_top > 0 && n_top < n) {
        for (int shift = 24; shift >= 0; shift -= 8) {
            for (int i = t; i < 256; i += SMP_THREADS) sm.hist[i] = 0u;
            __syncthreads();
            for (int base = 0; base < n; base += SMP_THREADS) {         // (every lane runs every trip: smp_hist_add is per wave)
                const int i = base + t;
                const unsigned key = i < n ? smp_key(x[i]) : 0u;
                smp_hist_add(sm, i < n && (key & mask) == prefix, (key >> shift) & 255u);
            }
            __syncthreads();
            smp_find_digit(kk, sm);
            const unsigned d = sm.word[0], rem = sm.word[1], cnt = sm.word[2];
            __syncthreads();
            prefix |= d << shift;
            mask |= 255u << shift;
            kk = rem;
            if (cnt == kk) break;                  // every element of this digit is a winner
            if (shift == 0) {
                // cnt > kk values equal the n_top-th: the kk of them with the lowest indices (select on 255 - index digit)
                unsigned imask = 0u, ipre = 0u;
                for (int sh = 24; sh >= 0; sh -= 8) {
                    for (int i = t; i < 256; i += SMP_THREADS) sm.hist[i] = 0u;
                    __syncthreads();
                    for (int i = t; i < n; i += SMP_THREADS)
                        if (smp_key(x[i]) == prefix && ((unsigned)i & imask) == ipre) atomicAdd(&sm.hist[255u - (((unsigned)i >> sh) & 255u)], 1u);
                    __syncthreads();
                    smp_find_digit(kk, sm);
                    const unsigned di = 255u - sm.word[0], ri = sm.word[1];
                    __syncthreads();
                    ipre |= di << sh;
                    imask |= 255u << sh;
                    kk = ri;
                }
                ilim = (int)ipre;
            }
        }
    }
    // 3. the winners into LDS (exactly n_win of them; the bound keeps a row outside the contract -- NaN -- inside the arrays)
    if (n_win > 0) {
        for (int i = t; i < n; i += SMP_THREADS) {
            const unsigned key = smp_key(x[i]);
            const unsigned km = key & mask;
            if (km > prefix || (km == prefix && i <= ilim)) {
                const unsigned slot = atomicAdd(&lps.count, 1u);
                if (slot < (unsigned)LP_TOP) { lps.key[slot] = key; lps.idx[slot] = i; }
            }
        }
    }
    __syncthreads();
    // 4. the record
    if (t < n_slots) {
        const int have = min((int)lps.count, min(n_win, LP_TOP));
        if (t < have) {
            const unsigned key = lps.key[t];
            const int idx = lps.idx[t];
            int place = 0;
            for (int j = 0; j < have; j++) place += (int)(lps.key[j] > key || (lps.key[j] == key && lps.idx[j] < idx));
            top_id[place] = idx;
            top_lp[place] = x[idx] - lse;
        } else {
            top_id[t] = -1;
            top_lp[t] = 0.f;
        }
    }
    if (t == 0) {
        if (lse_out) *lse_out = lse;
        *logprob_out = (id >= 0 && id < n) ? x[id] - lse : 0.f;
    }
}

// k_dec_sample / k_dec_sample_b for a decoder in which a sequence asked for log-probs: the same draw (bias0 null: no tables),
// then -- for a sequence whose request carries lp1 = n_top + 1 > 0 -- the record of position n, before the commit advances n.
// The choice is per workgroup, outside every pass.  rec0: [sequences][rec_stride] records.
__global__ __launch_bounds__(SMP_THREADS) void k_dec_sample_lp(const float* __restrict__ logits0, int n_vocab, int row_stride, const SampleParam* __restrict__ par0,
                                                              DecStep* step0, int32_t* __restrict__ result0, int result_stride,
                                                              int32_t* __restrict__ tokens0, int tok_stride, const float* __restrict__ bias0,
                                                              LpRecord* __restrict__ rec0, int rec_stride)
{
    __shared__ SmpShared sm;
    __shared__ LpShared lps;
    const SampleParam p = par0[blockIdx.x];
    DecStep* step = step0 + blockIdx.x;
    const unsigned pos = (unsigned)step->n;
    const float* x = logits0 + (size_t)blockIdx.x * row_stride;
    int idx;
    if (bias0 && p.table1 > 0 && (p.until == 0u || pos < p.until))
        idx = smp_row<true>(x, bias0 + (size_t)(p.table1 - 1) * (size_t)n_vocab, n_vocab, p.top_k, p.temp, pos, p.stream, p.seed_lo, p.seed_hi, sm);
    else
        idx = smp_row<false>(x, nullptr, n_vocab, p.top_k, p.temp, pos, p.stream, p.seed_lo, p.seed_hi, sm);
    if (p.lp1 > 0u && pos < (unsigned)rec_stride) {
        LpRecord* r = rec0 + (size_t)blockIdx.x * (size_t)rec_stride + pos;
        smp_logprobs_row(x, n_vocab, min((int)p.lp1 - 1, LP_TOP), idx, LP_TOP, &r->lse, &r->logprob, r->top_id, r->top_logprob, sm, lps);
    }
    if (threadIdx.x == 0) dec_pick_commit(step, result0 + (size_t)blockIdx.x * result_stride, tokens0 + (size_t)blockIdx.x * tok_stride, idx);
}

// gten_hip_row_top_logprobs: row r of the logits with the chosen id ids[r] (-1: none)
__global__ __launch_bounds__(SMP_THREADS) void k_row_top_logprobs(const float* __restrict__ logits, int n_vocab, long long row_stride,
                                                                 const int32_t* __restrict__ ids, int n_top, float* __restrict__ logprob_out,
                                                                 int32_t* __restrict__ top_id_out, float* __restrict__ top_lp_out)
{
    __shared__ SmpShared sm;
    __shared__ LpShared lps;
    const size_t r = blockIdx.x;
    smp_logprobs_row(logits + r * (size_t)row_stride, n_vocab, n_top, ids[r], n_top, nullptr, logprob_out + r, top_id_out + r * (size_t)n_top,
                     top_lp_out + r * (size_t)n_top, sm, lps);
}
