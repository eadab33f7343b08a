// gten_decode_nucleus.h -- top-p and min-p truncation of the draw as exact integer cuts, on the device (DESIGN.md §3.12,
// include/gten_hip_nucleus.h); included by gten_decode.hip behind gten_decode_logprobs.h, whose workgroup shape, key order,
// histogram helpers and record routine it uses.
//
// One workgroup of SMP_THREADS per row y (x, or x + b):
//   1. the candidates C: smp_row's radix select on smp_key (and on the indices where several values equal the k-th);
//   2. one pass over C: Z = sum q_j in u64 (q_j = floorf(expf(a_j) * 2^36), a_j = (y_j - max y) / temp) and
//      n_minp = #{a_j >= t}; per-thread partials, __shfl_xor across the wave, LDS across the waves -- integer sums;
//   3. top_p < 1: a second radix select over C, eight bits per pass, whose histogram holds u64 MASS per digit (LDS integer
//      atomics); scanning from digit 255 down until the running mass reaches P = floor((double)Z * top_p) leaves the cut key
//      and the mass still missing inside its run of equal keys; those have equal q, so ceil(missing / q) of them are taken,
//      the ones with the lowest indices (the index select of smp_row);
//   4. the draw of smp_row over the members of C that are inside the nucleus AND have a_j >= t -- the intersection of two
//      prefixes of C is the shorter one, the first n_keep = min(n_nucleus, n_minp).
// At most SMP_THREADS candidates (top_k <= 1024): steps 2-4 run on the candidates alone, one per thread, compacted into LDS -- each
// thread sums the masses of the candidates that precede its own and is inside the nucleus when that sum is below P.  The same
// integers, so the same ids; the row is read once more, not seven times.
// No float sum enters a decision: every count and every mass is an integer fact about the row.
#pragma once

#define CUT_MASS_BITS 36         // GTEN_HIP_NUCLEUS_MASS_BITS

struct CutParam {                // one sequence's cut (gten_hip_decoder_set_cut); 16 bytes
    float top_p;
    float t;                     // (float)log((double)min_p), formed on the host
    float min_p;
    unsigned on;                 // 0: no cut (top_p == 1 && min_p == 0, or never set) -- the sequence draws by smp_row
};
struct CutInfo {                 // gten_hip_cut_info; 24 bytes
    unsigned long long Z;
    int32_t n_cand, n_nucleus, n_minp, n_keep;
};
static_assert(sizeof(CutParam) == 16 && sizeof(CutInfo) == 24, "CutParam is 16 bytes, CutInfo 24 (include/gten_hip_nucleus.h)");

struct CutShared {
    unsigned long long cq[SMP_THREADS];      // at most SMP_THREADS candidates: mass, key, index of each (in no particular order)
    unsigned ckey[SMP_THREADS];
    int cidx[SMP_THREADS];
    unsigned long long mass[256];
    unsigned long long wz[SMP_WAVES];
    unsigned long long word[2];  // mass still missing inside the digit found, mass of that digit
    unsigned wc[SMP_WAVES];
    unsigned digit;
    unsigned count;
    unsigned have;
};

__device__ __forceinline__ float cut_score(float v, float mx, float temp) { return (v - mx) / temp; }

__device__ __forceinline__ unsigned long long cut_mass(float a)
{
    const float w = expf(a) * 0x1p36f;             // a <= 0: w in [0, 2^36], the multiply is exact
    return w > 0.f ? (unsigned long long)floorf(w) : 0ull;      // (a NaN -- outside the contract -- counts as nothing)
}

__device__ __forceinline__ float cut_unkey(unsigned k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// mass q of digit d from every lane with `on`; the whole wave calls it.  As smp_hist_add: the lanes that share the first
// active lane's digit add their sum in ONE atomic, the others add theirs one by one.
__device__ __forceinline__ void cut_mass_add(CutShared& cs, bool on, unsigned d, unsigned long long q)
{
    const unsigned long long act = __ballot(on);
    if (act == 0ull) return;
    const int lead = __ffsll((long long)act) - 1, lane = threadIdx.x & 63;
    const unsigned d0 = (unsigned)__shfl((int)d, lead, 64);
    const bool mine = on && d == d0;
    unsigned long long s = mine ? q : 0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == lead) atomicAdd(&cs.mass[d0], s);
    else if (on && !mine) atomicAdd(&cs.mass[d], q);
}

// cs.mass holds the mass of 256 digits; find the digit d, scanning from 255 down, at which the running mass reaches `need`
// (>= 1); afterwards cs.digit = d, cs.word = {need - (mass above d), mass of d}.  Wave 0 scans, as in smp_find_digit.
__device__ __forceinline__ void cut_find_digit(unsigned long long need, CutShared& cs)
{
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        const unsigned long long h0 = cs.mass[255 - 4 * lane], h1 = cs.mass[254 - 4 * lane], h2 = cs.mass[253 - 4 * lane], h3 = cs.mass[252 - 4 * lane];
        const unsigned long long c = h0 + h1 + h2 + h3;
        unsigned long long incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long u = __shfl_up(incl, o, 64);
            if (lane >= o) incl += u;
        }
        const unsigned long long excl = incl - c;
        if (excl < need && incl >= need) {            // exactly one lane
            unsigned long long above = excl, h = h0;
            unsigned d = 255 - 4 * lane;
            if (above + h < need) { above += h; d--; h = h1;
                if (above + h < need) { above += h; d--; h = h2;
                    if (above + h < need) { above += h; d--; h = h3; } } }
            cs.digit = d; cs.word[0] = need - above; cs.word[1] = h;
        }
    }
    __syncthreads();
}

// One row under a cut: the id of the contract (top_k >= 1; the caller sends greedy rows to smp_row).  Every thread returns
// it; thread 0 writes *info when info is not null.  top_p in (0, 1], t <= 0 (-inf: no min-p).
template <bool BIAS, bool PEN = false, bool FSM = false>
__device__ __forceinline__ int smp_row_cut(const float* __restrict__ x, const float* __restrict__ b, int n, int top_k, float temp, unsigned pos,
                                           unsigned stream, unsigned k0, unsigned k1, float top_p, float tmin, CutInfo* __restrict__ info,
                                           SmpShared& sm, CutShared& cs, const PenRow& pen = PenRow{}, const FsmRow& fsm = FsmRow{})
{
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    // 1. the candidates, as smp_row finds them: (key & mask) > prefix, or == prefix with index <= ilim
    const SmpSelect sel = smp_select<BIAS, PEN, FSM>(x, b, n, top_k, sm, pen, fsm);
    const unsigned mask = sel.mask, prefix = sel.prefix;
    const int ilim = sel.ilim, n_cand = min(top_k, n);
    const float mx = sel.mx;
    unsigned kk;
    const bool cutting = top_p < 1.f;
    if (n_cand <= SMP_THREADS) {
        // 2'-4'. one candidate per thread
        if (t == 0) { cs.have = 0u; cs.count = 0u; }
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
        unsigned c = (unsigned)(mine && a >= tmin);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { z += __shfl_xor(z, o, 64); c += __shfl_xor(c, o, 64); }
        if (lane == 0) { cs.wz[wid] = z; cs.wc[wid] = c; }
        __syncthreads();
        unsigned long long Z = 0ull;
        unsigned n_minp = 0u;
        for (int w = 0; w < SMP_WAVES; w++) { Z += cs.wz[w]; n_minp += cs.wc[w]; }
        bool in = mine;
        if (cutting) {
            unsigned long long need = (unsigned long long)floor((double)Z * (double)top_p);
            if (need == 0ull) need = 1ull;         // the shortest NON-EMPTY prefix: the maximum's q is 2^36
            unsigned long long before = 0ull;      // the mass of the candidates that precede this one
            for (int j = 0; j < have; j++) {
                const unsigned kj = cs.ckey[j];
                if (kj > key || (kj == key && cs.cidx[j] < ci)) before += cs.cq[j];
            }
            in = mine && before < need;
        }
        float best = -INFINITY;
        int idx = 0x7fffffff;
        if (in && a >= tmin) { best = a + smp_gumbel((unsigned)ci, pos, stream, k0, k1); idx = ci; }
        if (info) {
            unsigned m = (unsigned)in;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) m += __shfl_xor(m, o, 64);
            if (lane == 0) atomicAdd(&cs.count, m);
        }
        idx = smp_block_argmax(best, idx, sm);     // (its barriers order cs.count)
        if (info && t == 0) {
            const int n_nuc = (int)cs.count;
            info->Z = Z; info->n_cand = n_cand; info->n_nucleus = n_nuc; info->n_minp = (int)n_minp; info->n_keep = min(n_nuc, (int)n_minp);
        }
        return idx;
    }
    // 2. Z and n_minp over C
    unsigned long long Z = 0ull;
    unsigned n_minp = 0u;
    {
        unsigned long long z = 0ull;
        unsigned c = 0u;
        for (int i = t; i < n; i += SMP_THREADS) {
            const float v = smp_at<BIAS, PEN, FSM>(x, b, i, pen, fsm);
            const unsigned km = smp_key(v) & mask;
            if (km > prefix || (km == prefix && i <= ilim)) {
                const float a = cut_score(v, mx, temp);
                c += (unsigned)(a >= tmin);
                if (cutting || info) z += cut_mass(a);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { z += __shfl_xor(z, o, 64); c += __shfl_xor(c, o, 64); }
        if (lane == 0) { cs.wz[wid] = z; cs.wc[wid] = c; }
        if (t == 0) cs.count = 0u;
        __syncthreads();
        for (int w = 0; w < SMP_WAVES; w++) { Z += cs.wz[w]; n_minp += cs.wc[w]; }
    }
    // 3. the nucleus: key > ckey, or == ckey with index <= clim
    unsigned ckey = 0u;
    int clim = 0x7fffffff;
    if (cutting) {
        unsigned long long need = (unsigned long long)floor((double)Z * (double)top_p);
        if (need == 0ull) need = 1ull;             // the shortest NON-EMPTY prefix: the maximum's q is 2^36
        unsigned cmask = 0u;
        for (int shift = 24; shift >= 0; shift -= 8) {
            for (int i = t; i < 256; i += SMP_THREADS) cs.mass[i] = 0ull;
            __syncthreads();
            for (int base = 0; base < n; base += SMP_THREADS) {         // (every lane runs every trip: cut_mass_add is per wave)
                const int i = base + t;
                const float v = i < n ? smp_at<BIAS, PEN, FSM>(x, b, i, pen, fsm) : -INFINITY;
                const unsigned key = smp_key(v), km = key & mask;
                const bool cand = i < n && (km > prefix || (km == prefix && i <= ilim));
                const unsigned long long q = cand && (key & cmask) == ckey ? cut_mass(cut_score(v, mx, temp)) : 0ull;
                cut_mass_add(cs, q > 0ull, (key >> shift) & 255u, q);
            }
            __syncthreads();
            cut_find_digit(need, cs);
            const unsigned d = cs.digit;
            need = cs.word[0];
            __syncthreads();
            ckey |= d << shift;
            cmask |= 255u << shift;
        }
        // `need` of the run's mass is still missing; every member of the run has the same q
        unsigned long long q = cut_mass(cut_score(cut_unkey(ckey), mx, temp));
        if (q == 0ull) q = 1ull;
        kk = (unsigned)((need + q - 1ull) / q);
        unsigned imask = 0u, ipre = 0u;
        for (int s = 8; s >= 0; s -= 8) {
            for (int i = t; i < 256; i += SMP_THREADS) sm.hist[i] = 0u;
            __syncthreads();
            for (int i = t; i < n; i += SMP_THREADS) {
                const unsigned key = smp_key(smp_at<BIAS, PEN, FSM>(x, b, i, pen, fsm)), km = key & mask;
                if (key == ckey && (km > prefix || i <= ilim) && ((unsigned)i & imask) == ipre) atomicAdd(&sm.hist[255u - (((unsigned)i >> s) & 255u)], 1u);
            }
            __syncthreads();
            smp_find_digit(kk, sm);
            const unsigned di = 255u - sm.word[0], ri = sm.word[1];
            __syncthreads();
            ipre |= di << s;
            imask |= 255u << s;
            kk = ri;
        }
        clim = (int)ipre;
    }
    // 4. the draw over the first min(n_nucleus, n_minp) of C
    float best = -INFINITY;
    int idx = 0x7fffffff;
    unsigned c = 0u;
    for (int i = t; i < n; i += SMP_THREADS) {
        const float v = smp_at<BIAS, PEN, FSM>(x, b, i, pen, fsm);
        const unsigned key = smp_key(v), km = key & mask;
        if (km > prefix || (km == prefix && i <= ilim)) {
            const bool in = key > ckey || (key == ckey && i <= clim);
            c += (unsigned)in;
            const float a = cut_score(v, mx, temp);
            if (in && a >= tmin) {
                const float s = a + smp_gumbel((unsigned)i, pos, stream, k0, k1);
                if (s > best || (s == best && i < idx)) { best = s; idx = i; }
            }
        }
    }
    if (info) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if (lane == 0) atomicAdd(&cs.count, c);
    }
    idx = smp_block_argmax(best, idx, sm);         // (its barriers order cs.count)
    if (info && t == 0) {
        const int n_nuc = (int)cs.count;
        info->Z = Z; info->n_cand = n_cand; info->n_nucleus = n_nuc; info->n_minp = (int)n_minp; info->n_keep = min(n_nuc, (int)n_minp);
    }
    return idx;
}

// k_dec_sample_lp for a decoder in which a sequence has set a cut (cut0: [sequences]): a sampling sequence whose cut is on draws
// by smp_row_cut -- under its bias table where one holds --, every other one exactly as k_dec_sample_lp does; then the record of
// a sequence that asks for log-probs (rec0 null: nobody ever asked).  The choice is per workgroup, outside every pass.
__global__ __launch_bounds__(SMP_THREADS) void k_dec_sample_cut(const float* __restrict__ logits0, int n_vocab, int row_stride, const SampleParam* __restrict__ par0,
                                                               DecStep* step0, int32_t* __restrict__ result0, int result_stride,
                                                               int32_t* __restrict__ tokens0, int tok_stride, const float* __restrict__ bias0,
                                                               LpRecord* __restrict__ rec0, int rec_stride, const CutParam* __restrict__ cut0)
{
    __shared__ SmpShared sm;
    __shared__ LpShared lps;
    __shared__ CutShared cs;
    const SampleParam p = par0[blockIdx.x];
    const CutParam c = cut0[blockIdx.x];
    DecStep* step = step0 + blockIdx.x;
    const unsigned pos = (unsigned)step->n;
    const float* x = logits0 + (size_t)blockIdx.x * row_stride;
    const bool biased = bias0 && p.table1 > 0 && (p.until == 0u || pos < p.until);
    const float* b = biased ? bias0 + (size_t)(p.table1 - 1) * (size_t)n_vocab : nullptr;
    int idx;
    if (c.on != 0u && p.top_k > 0) {
        if (biased) idx = smp_row_cut<true>(x, b, n_vocab, p.top_k, p.temp, pos, p.stream, p.seed_lo, p.seed_hi, c.top_p, c.t, nullptr, sm, cs);
        else idx = smp_row_cut<false>(x, nullptr, n_vocab, p.top_k, p.temp, pos, p.stream, p.seed_lo, p.seed_hi, c.top_p, c.t, nullptr, sm, cs);
    } else {
        if (biased) idx = smp_row<true>(x, b, n_vocab, p.top_k, p.temp, pos, p.stream, p.seed_lo, p.seed_hi, sm);
        else idx = smp_row<false>(x, nullptr, n_vocab, p.top_k, p.temp, pos, p.stream, p.seed_lo, p.seed_hi, sm);
    }
    if (rec0 && p.lp1 > 0u && pos < (unsigned)rec_stride) {
        LpRecord* r = rec0 + (size_t)blockIdx.x * (size_t)rec_stride + pos;
        smp_logprobs_row(x, n_vocab, min((int)p.lp1 - 1, LP_TOP), idx, LP_TOP, &r->lse, &r->logprob, r->top_id, r->top_logprob, sm, lps);
    }
    if (threadIdx.x == 0) dec_pick_commit(step, result0 + (size_t)blockIdx.x * result_stride, tokens0 + (size_t)blockIdx.x * tok_stride, idx);
}

// gten_hip_sample_rows_cut: row r of the logits (bias null: y = x), its own request and cut.  A greedy row, and a row without a
// cut when no info is asked for, draws by smp_row (info: zeros for a greedy row).
__global__ __launch_bounds__(SMP_THREADS) void k_sample_rows_cut(const float* __restrict__ logits, int n_vocab, long long row_stride,
                                                                const float* __restrict__ bias, long long bias_stride,
                                                                const SampleRowParam* __restrict__ par, const CutParam* __restrict__ cut,
                                                                unsigned seed_lo, unsigned seed_hi, int32_t* __restrict__ out, CutInfo* __restrict__ info)
{
    __shared__ SmpShared sm;
    __shared__ CutShared cs;
    const SampleRowParam p = par[blockIdx.x];
    const CutParam c = cut[blockIdx.x];
    const float* x = logits + (size_t)blockIdx.x * (size_t)row_stride;
    const float* b = bias ? bias + (size_t)blockIdx.x * (size_t)bias_stride : nullptr;
    CutInfo* inf = info ? info + blockIdx.x : nullptr;
    int idx;
    if (p.top_k > 0 && (c.on != 0u || inf)) {
        if (b) idx = smp_row_cut<true>(x, b, n_vocab, p.top_k, p.temp, p.pos, p.stream, seed_lo, seed_hi, c.top_p, c.t, inf, sm, cs);
        else idx = smp_row_cut<false>(x, nullptr, n_vocab, p.top_k, p.temp, p.pos, p.stream, seed_lo, seed_hi, c.top_p, c.t, inf, sm, cs);
    } else {
        if (b) idx = smp_row<true>(x, b, n_vocab, p.top_k, p.temp, p.pos, p.stream, seed_lo, seed_hi, sm);
        else idx = smp_row<false>(x, nullptr, n_vocab, p.top_k, p.temp, p.pos, p.stream, seed_lo, seed_hi, sm);
        if (inf && threadIdx.x == 0) { inf->Z = 0ull; inf->n_cand = 0; inf->n_nucleus = 0; inf->n_minp = 0; inf->n_keep = 0; }
    }
    if (threadIdx.x == 0) out[blockIdx.x] = idx;
}
