// gten_decode_sample.h -- top-k sampling with a temperature on the device, included by gten_decode.hip.
//
// One workgroup of SMP_THREADS per logits row:
//   1. the candidates are the k largest logits, ties at the k-th value to the lower index: a radix select, eight bits per
//      pass, on the order-preserving integer image of the f32 logits (and, only where several logits equal the k-th
//      value, a second select on their indices) -- exact, no float arithmetic;
//   2. each candidate j gets Gumbel noise g_j from Philox4x32-10 at counter (j, position, stream, 0), key = the seed;
//   3. the id is the argmax over the candidates of (x_j - max x) / temp + g_j, the lower index winning ties.
// This is a draw from softmax(x / temp) restricted to the top k (the Gumbel-max trick) in which no sort, prefix sum or
// float reduction order enters the result.  top_k == 0 is k_dec_argmax's rule over the whole row.
#pragma once

#define SMP_THREADS 1024
#define SMP_WAVES (SMP_THREADS / 64)

struct SampleParam {             // one sequence's request (gten_hip_decoder_set_sampling); 32 bytes
    int top_k;                   // 0: greedy
    float temp;
    unsigned stream;
    unsigned seed_lo, seed_hi;
    int table1;                  // bias table + 1 (0: none), so that a zeroed request is "greedy, no table"
    unsigned until;              // the table holds for positions < until (0: for every position)
    unsigned lp1;                // log-prob request n_top + 1 (0: none), read by k_dec_sample_lp only (gten_decode_logprobs.h)
};
struct SampleRowParam {          // one row of gten_hip_sample_rows; 16 bytes
    int top_k;
    float temp;
    unsigned stream, pos;
};

__device__ __forceinline__ unsigned smp_key(float f)
{
    unsigned u = __float_as_uint(f);
    if (u == 0x80000000u) u = 0u;                             // -0 == +0: one key, so a tie between them goes by index
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);       // larger float -> larger key
}

// word 0 of Philox4x32-10 (Random123) at counter (c0, c1, c2, 0), key (k0, k1)
__device__ __forceinline__ unsigned smp_philox0(unsigned c0, unsigned c1, unsigned c2, unsigned k0, unsigned k1)
{
    unsigned c3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const unsigned lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
        const unsigned lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}

// Gumbel noise of index j: u = f32((w >> 8) + 0.5) * 2^-24 (f32 rounding for u >= 1/2), capped at 1 - 2^-24 so that
// -log(u) > 0; g = -log(-log(u))
__device__ __forceinline__ float smp_gumbel(unsigned j, unsigned pos, unsigned stream, unsigned k0, unsigned k1)
{
    const unsigned w = smp_philox0(j, pos, stream, k0, k1);
    float u = ((float)(w >> 8) + 0.5f) * 0x1p-24f;
    u = fminf(u, 0x1.fffffep-1f);
    return -logf(-logf(u));
}

struct SmpShared {
    unsigned hist[256];
    float rv[SMP_WAVES];
    int ri[SMP_WAVES];
    unsigned word[4];            // digit found, remaining rank, count of that digit
};

// (value, index) argmax across the workgroup, strict '>' then the lower index; every thread returns the winner
__device__ __forceinline__ int smp_block_argmax(float best, int idx, SmpShared& sm)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (ov > best || (ov == best && oi < idx)) { best = ov; idx = oi; }
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) { sm.rv[wid] = best; sm.ri[wid] = idx; }
    __syncthreads();
    best = sm.rv[0]; idx = sm.ri[0];
    for (int w = 1; w < SMP_WAVES; w++)
        if (sm.rv[w] > best || (sm.rv[w] == best && sm.ri[w] < idx)) { best = sm.rv[w]; idx = sm.ri[w]; }
    return idx == 0x7fffffff ? 0 : idx;
}

__device__ __forceinline__ float smp_block_max(float m, SmpShared& sm)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) sm.rv[wid] = m;
    __syncthreads();
    m = sm.rv[0];
    for (int w = 1; w < SMP_WAVES; w++) m = fmaxf(m, sm.rv[w]);
    __syncthreads();
    return m;
}

// one histogram count per lane with `on`, digit d; the whole wave calls it.  The logits of a row crowd into few digits (the
// top byte of a key is the sign and seven exponent bits), and same-address LDS atomics of one instruction serialise: the
// lanes that share the first active lane's digit add their count in ONE atomic, the others add theirs one by one.
__device__ __forceinline__ void smp_hist_add(SmpShared& sm, bool on, unsigned d)
{
    const unsigned long long act = __ballot(on);
    if (act == 0ull) return;
    const int lead = __ffsll((long long)act) - 1, lane = threadIdx.x & 63;
    const unsigned d0 = (unsigned)__shfl((int)d, lead, 64);
    const unsigned long long same = __ballot(on && d == d0);
    if (lane == lead) atomicAdd(&sm.hist[d0], (unsigned)__popcll(same));
    else if (on && d != d0) atomicAdd(&sm.hist[d], 1u);
}

// sm.hist holds a histogram of 256 digits; find the digit d, scanning from 255 down, at which the running count reaches
// `kk`; afterwards sm.word = {d, kk - (count above d), count of d}.  Wave 0 scans (lane l holds digits 255-4l .. 252-4l).
__device__ __forceinline__ void smp_find_digit(unsigned kk, SmpShared& sm)
{
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        const unsigned h0 = sm.hist[255 - 4 * lane], h1 = sm.hist[254 - 4 * lane], h2 = sm.hist[253 - 4 * lane], h3 = sm.hist[252 - 4 * lane];
        const unsigned c = h0 + h1 + h2 + h3;
        unsigned incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        const unsigned excl = incl - c;
        if (excl < kk && incl >= kk) {            // exactly one lane
            unsigned above = excl, d = 255 - 4 * lane, h = h0;
            if (above + h < kk) { above += h; d--; h = h1;
                if (above + h < kk) { above += h; d--; h = h2;
                    if (above + h < kk) { above += h; d--; h = h3; } } }
            sm.word[0] = d; sm.word[1] = kk - above; sm.word[2] = h;
        }
    }
    __syncthreads();
}

// element i of the row the draw is made from: the logit, or (BIAS) y_i = x_i + b_i -- one f32 add, formed anew
// wherever the row is read (the add is deterministic: every pass sees the same y)
//
// PEN (include/gten_hip_penalty.h): the logit is first penalised by the count c_i of id i in the sequence's window,
// p_i = x_i for c_i == 0, otherwise (x_i > 0 ? x_i / r : x_i * r) - ((float)c_i * freq + pres), every operation rounded to f32 on its
// own; then the table, y_i = p_i + b_i.  The counts are dense u16, two per LDS word (pen_count, gten_decode_penalty.h).  An instance
// without PEN never touches `pen`.
struct PenRow {
    const unsigned* cnt;         // LDS: (n_vocab + 1) / 2 words, id i in half (i & 1) of word i >> 1
    float r, freq, pres;
};
__device__ __forceinline__ float pen_apply(float x, unsigned c, const PenRow& pen)
{
    if (c == 0u) return x;
    const float u = x > 0.f ? __fdiv_rn(x, pen.r) : __fmul_rn(x, pen.r);
    const float t = __fadd_rn(__fmul_rn((float)c, pen.freq), pen.pres);
    return __fsub_rn(u, t);
}
//
// FSM (include/gten_hip_fsm.h): the mask form.  `fsm.next` is the row of the sequence's state in the automaton pool,
// one u16 per id; where it says FSM_DEAD the element is -inf, otherwise it is the element of the form below, bits untouched -- the
// penalty first, the mask second.  One u16 load per element read.  An instance without FSM never touches `fsm`.
#define FSM_DEAD 0xFFFFu
struct FsmRow {
    const uint16_t* next;        // next[i]: the state after id i, or FSM_DEAD
};
template <bool BIAS, bool PEN = false, bool FSM = false>
__device__ __forceinline__ float smp_at(const float* __restrict__ x, const float* __restrict__ b, int i, const PenRow& pen = PenRow{},
                                        const FsmRow& fsm = FsmRow{})
{
    if constexpr (FSM) {
        const float p = smp_at<BIAS, PEN, false>(x, b, i, pen);
        return fsm.next[i] == FSM_DEAD ? -INFINITY : p;
    } else if constexpr (PEN) {
        const float p = pen_apply(x[i], (pen.cnt[i >> 1] >> ((i & 1) << 4)) & 0xffffu, pen);
        if constexpr (BIAS) return __fadd_rn(p, b[i]);
        else return p;
    } else {
        if constexpr (BIAS) return x[i] + b[i];
        else return x[i];
    }
}

// The candidates of one row (top_k >= 1): element i is one when (smp_key(y_i) & mask) > prefix, or == prefix with i <= ilim; mx = max y.
// Every thread returns the same four values.  (smp_row and, under a cut, smp_row_cut of gten_decode_nucleus.h draw from them.)
struct SmpSelect {
    unsigned mask, prefix;
    int ilim;
    float mx;
};
template <bool BIAS, bool PEN = false, bool FSM = false>
__device__ __forceinline__ SmpSelect smp_select(const float* __restrict__ x, const float* __restrict__ b, int n, int top_k, SmpShared& sm,
                                                const PenRow& pen = PenRow{}, const FsmRow& fsm = FsmRow{})
{
    const int t = threadIdx.x;
    unsigned mask = 0u, prefix = 0u, kk = (unsigned)min(top_k, n);
    int ilim = 0x7fffffff;
    float mx = -INFINITY;
    const bool all = top_k >= n;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = t; i < 256; i += SMP_THREADS) sm.hist[i] = 0u;
        __syncthreads();
        if (shift == 24) {
            for (int base = 0; base < n; base += SMP_THREADS) {         // (every lane runs every trip: smp_hist_add is per wave)
                const int i = base + t;
                const float v = i < n ? smp_at<BIAS, PEN, FSM>(x, b, i, pen, fsm) : -INFINITY;
                mx = fmaxf(mx, v);
                if (!all) smp_hist_add(sm, i < n, smp_key(v) >> 24);
            }
            mx = smp_block_max(mx, sm);
            if (all) break;
        } else {
            for (int base = 0; base < n; base += SMP_THREADS) {
                const int i = base + t;
                const unsigned key = i < n ? smp_key(smp_at<BIAS, PEN, FSM>(x, b, i, pen, fsm)) : 0u;
                smp_hist_add(sm, i < n && (key & mask) == prefix, (key >> shift) & 255u);
            }
            __syncthreads();
        }
        smp_find_digit(kk, sm);
        const unsigned d = sm.word[0], rem = sm.word[1], cnt = sm.word[2];
        __syncthreads();
        prefix |= d << shift;
        mask |= 255u << shift;
        kk = rem;
        if (cnt == kk) break;                      // every element of this digit is a candidate: no narrower threshold needed
        if (shift == 0) {
            // cnt > kk logits equal the k-th value: the kk of them with the lowest indices (select on 255 - index digit)
            unsigned imask = 0u, ipre = 0u;
            for (int s = 8; s >= 0; s -= 8) {
                for (int i = t; i < 256; i += SMP_THREADS) sm.hist[i] = 0u;
                __syncthreads();
                for (int i = t; i < n; i += SMP_THREADS)
                    if (smp_key(smp_at<BIAS, PEN, FSM>(x, b, i, pen, fsm)) == prefix && ((unsigned)i & imask) == ipre) atomicAdd(&sm.hist[255u - (((unsigned)i >> s) & 255u)], 1u);
                __syncthreads();
                smp_find_digit(kk, sm);
                const unsigned di = 255u - sm.word[0], ri = sm.word[1];
                __syncthreads();
                ipre |= di << s;
                imask |= 255u << s;
                kk = ri;
            }
            ilim = (int)ipre;                       // the kk-th lowest index among the ties (indices < 65536)
        }
    }
    return SmpSelect{mask, prefix, ilim, mx};
}

// One row: the id of the contract (top_k >= 1) or the greedy argmax (top_k == 0).  Every thread returns it.
// BIAS: the row is y = x + b (b: a bias table's row; -inf = banned -- its key sorts below every finite value and its score is
// -inf, so it is never the argmax while one entry is above -inf); the unbiased instance never touches b.
template <bool BIAS, bool PEN = false, bool FSM = false>
__device__ __forceinline__ int smp_row(const float* __restrict__ x, const float* __restrict__ b, int n, int top_k, float temp, unsigned pos,
                                       unsigned stream, unsigned k0, unsigned k1, SmpShared& sm, const PenRow& pen = PenRow{},
                                       const FsmRow& fsm = FsmRow{})
{
    const int t = threadIdx.x;
    if (top_k <= 0) {
        float best = -INFINITY;
        int idx = 0x7fffffff;
        for (int i = t; i < n; i += SMP_THREADS) {
            const float v = smp_at<BIAS, PEN, FSM>(x, b, i, pen, fsm);
            if (v > best || (v == best && i < idx)) { best = v; idx = i; }
        }
        return smp_block_argmax(best, idx, sm);
    }
    const SmpSelect c = smp_select<BIAS, PEN, FSM>(x, b, n, top_k, sm, pen, fsm);
    const unsigned mask = c.mask, prefix = c.prefix;
    const int ilim = c.ilim;
    const float mx = c.mx;
    float best = -INFINITY;
    int idx = 0x7fffffff;
    for (int i = t; i < n; i += SMP_THREADS) {
        const float v = smp_at<BIAS, PEN, FSM>(x, b, i, pen, fsm);
        const unsigned key = smp_key(v) & mask;
        if (key > prefix || (key == prefix && i <= ilim)) {
            const float s = (v - mx) / temp + smp_gumbel((unsigned)i, pos, stream, k0, k1);
            if (s > best || (s == best && i < idx)) { best = s; idx = i; }
        }
    }
    return smp_block_argmax(best, idx, sm);
}

// the last launch of a sampled decode step: one workgroup per sequence of the lane, its logits row at logits0 + seq * stride;
// the position of the id is the step's n (the id that will sit at position n)
__global__ __launch_bounds__(SMP_THREADS) void k_dec_sample(const float* __restrict__ logits0, int n_vocab, int row_stride, const SampleParam* __restrict__ par0,
                                                           DecStep* step0, int32_t* __restrict__ result0, int result_stride,
                                                           int32_t* __restrict__ tokens0, int tok_stride)
{
    __shared__ SmpShared sm;
    const SampleParam p = par0[blockIdx.x];
    DecStep* step = step0 + blockIdx.x;
    const unsigned pos = (unsigned)step->n;
    const int idx = smp_row<false>(logits0 + (size_t)blockIdx.x * row_stride, nullptr, n_vocab, p.top_k, p.temp, pos, p.stream, p.seed_lo, p.seed_hi, sm);
    if (threadIdx.x == 0) dec_pick_commit(step, result0 + (size_t)blockIdx.x * result_stride, tokens0 + (size_t)blockIdx.x * tok_stride, idx);
}

// gten_hip_sample_rows: row r of the logits, its own request, one seed
__global__ __launch_bounds__(SMP_THREADS) void k_sample_rows(const float* __restrict__ logits, int n_vocab, long long row_stride,
                                                            const SampleRowParam* __restrict__ par, unsigned seed_lo, unsigned seed_hi, int32_t* __restrict__ out)
{
    __shared__ SmpShared sm;
    const SampleRowParam p = par[blockIdx.x];
    const int idx = smp_row<false>(logits + (size_t)blockIdx.x * (size_t)row_stride, nullptr, n_vocab, p.top_k, p.temp, p.pos, p.stream, seed_lo, seed_hi, sm);
    if (threadIdx.x == 0) out[blockIdx.x] = idx;
}

// ---- bias tables (include/gten_hip_bias.h).  k_dec_sample with the decoder's tables: a sequence whose request
// names a table (table1 > 0) that still holds at this position draws from y = x + b, every other one exactly as k_dec_sample does
// -- the choice is per workgroup, outside the select.  bias0: [tables][n_vocab] f32.
__global__ __launch_bounds__(SMP_THREADS) void k_dec_sample_b(const float* __restrict__ logits0, int n_vocab, int row_stride, const SampleParam* __restrict__ par0,
                                                             DecStep* step0, int32_t* __restrict__ result0, int result_stride,
                                                             int32_t* __restrict__ tokens0, int tok_stride, const float* __restrict__ bias0)
{
    __shared__ SmpShared sm;
    const SampleParam p = par0[blockIdx.x];
    DecStep* step = step0 + blockIdx.x;
    const unsigned pos = (unsigned)step->n;
    const float* x = logits0 + (size_t)blockIdx.x * row_stride;
    int idx;
    if (p.table1 > 0 && (p.until == 0u || pos < p.until))
        idx = smp_row<true>(x, bias0 + (size_t)(p.table1 - 1) * (size_t)n_vocab, n_vocab, p.top_k, p.temp, pos, p.stream, p.seed_lo, p.seed_hi, sm);
    else
        idx = smp_row<false>(x, nullptr, n_vocab, p.top_k, p.temp, pos, p.stream, p.seed_lo, p.seed_hi, sm);
    if (threadIdx.x == 0) dec_pick_commit(step, result0 + (size_t)blockIdx.x * result_stride, tokens0 + (size_t)blockIdx.x * tok_stride, idx);
}

// gten_hip_sample_rows_biased: k_sample_rows on y = x + b, row r's bias at bias + r * bias_stride (0: one row for all)
__global__ __launch_bounds__(SMP_THREADS) void k_sample_rows_b(const float* __restrict__ logits, int n_vocab, long long row_stride,
                                                              const float* __restrict__ bias, long long bias_stride,
                                                              const SampleRowParam* __restrict__ par, unsigned seed_lo, unsigned seed_hi, int32_t* __restrict__ out)
{
    __shared__ SmpShared sm;
    const SampleRowParam p = par[blockIdx.x];
    const int idx = smp_row<true>(logits + (size_t)blockIdx.x * (size_t)row_stride, bias + (size_t)blockIdx.x * (size_t)bias_stride, n_vocab, p.top_k, p.temp,
                                  p.pos, p.stream, seed_lo, seed_hi, sm);
    if (threadIdx.x == 0) out[blockIdx.x] = idx;
}
