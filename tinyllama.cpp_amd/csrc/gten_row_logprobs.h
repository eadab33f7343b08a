// gten_row_logprobs.h -- k_row_logprobs, the kernel of gten_hip_row_logprobs (include/gten_hip_score.h); included by
// gten_ops.hip.
#pragma once

#include "gten_dev.h"

// log-softmax of f32 logits rows read at one target id per row.
// One workgroup of 256 threads per row, one pass over it.  Each thread walks its elements in ascending order and keeps
//   m, s : the running maximum and sum of exp(x - m) (rescaled when m grows; exp as exp2 of (x - m) * log2 e)
//   c    : how many of its elements rank ahead of the target (x > x_t, or x == x_t at a lower index)
//   bi   : the index of its first maximum (strict >: the greedy rule of k_argmax_row)
// then the states are merged across the 64 lanes of a wave and across the 4 waves through LDS.
namespace {
constexpr int LP_THREADS = 256;
constexpr float LP_LOG2E = 1.4426950408889634f;

struct LpState {
    float m, s;
    int c, bi;
};

__device__ inline float lp_exp(float d) { return __builtin_amdgcn_exp2f(d * LP_LOG2E); }   // d <= 0

// an empty state (m = -inf, s = 0) merges without NaN: its term is skipped, not formed as 0 * exp(-inf + inf)
__device__ inline void lp_merge(LpState& a, float om, float os, int oc, int obi)
{
    const float mn = fmaxf(a.m, om);
    const float sa = a.s == 0.f ? 0.f : a.s * lp_exp(a.m - mn);
    const float sb = os == 0.f ? 0.f : os * lp_exp(om - mn);
    if (om > a.m || (om == a.m && obi < a.bi)) a.bi = obi;
    a.m = mn;
    a.s = sa + sb;
    a.c += oc;
}

// four consecutive elements j0 .. j0 + 3 (the tail passes -inf for missing ones: no term, no rank, never a maximum)
__device__ inline void lp_step4(LpState& a, float x0, float x1, float x2, float x3, int j0, float xt, int t)
{
    const float mx = fmaxf(fmaxf(x0, x1), fmaxf(x2, x3));
    const int fi = x0 == mx ? 0 : (x1 == mx ? 1 : (x2 == mx ? 2 : 3));
    if (mx > a.m) a.bi = j0 + fi;
    const float mn = fmaxf(a.m, mx);
    a.s = a.s * lp_exp(a.m - mn) + ((lp_exp(x0 - mn) + lp_exp(x1 - mn)) + (lp_exp(x2 - mn) + lp_exp(x3 - mn)));
    a.m = mn;
    a.c += (int)(x0 > xt || (x0 == xt && j0 < t)) + (int)(x1 > xt || (x1 == xt && j0 + 1 < t)) +
           (int)(x2 > xt || (x2 == xt && j0 + 2 < t)) + (int)(x3 > xt || (x3 == xt && j0 + 3 < t));
}

__device__ inline void lp_step1(LpState& a, float x, int j, float xt, int t)
{
    if (x > a.m) a.bi = j;
    const float mn = fmaxf(a.m, x);
    a.s = a.s * lp_exp(a.m - mn) + lp_exp(x - mn);
    a.m = mn;
    a.c += (int)(x > xt || (x == xt && j < t));
}
} // namespace

// VEC: the row base is 16-byte aligned (base and row_stride % 4 == 0): float4 loads, four per thread in flight, a scalar tail
template <bool VEC>
__global__ __launch_bounds__(LP_THREADS) void k_row_logprobs(const float* __restrict__ logits, int n_vocab, long long row_stride,
                                                             const int32_t* __restrict__ targets, float* __restrict__ lp_out,
                                                             int32_t* __restrict__ rank_out, int32_t* __restrict__ argmax_out)
{
    const int row = blockIdx.x, tid = threadIdx.x;
    const float* __restrict__ x = logits + (size_t)row * (size_t)row_stride;
    const int t_in = targets[row];
    const bool scored = t_in >= 0 && t_in < n_vocab;
    if (!scored && !argmax_out) {
        if (tid == 0) {
            lp_out[row] = 0.f;
            if (rank_out) rank_out[row] = -1;
        }
        return;
    }
    // the target's value, read once (a uniform load) and held by every lane; an unscored row counts nothing (x > +inf never)
    const int t = scored ? t_in : -1;
    const float xt = scored ? x[t] : INFINITY;
    LpState a{-INFINITY, 0.f, 0, 0x7fffffff};
    if constexpr (VEC) {
        const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x);
        const int n4 = n_vocab >> 2;
        int i = tid;
        for (; i + 3 * LP_THREADS < n4; i += 4 * LP_THREADS) {
            float4 v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = x4[i + k * LP_THREADS];
#pragma unroll
            for (int k = 0; k < 4; k++) lp_step4(a, v[k].x, v[k].y, v[k].z, v[k].w, 4 * (i + k * LP_THREADS), xt, t);
        }
        for (; i < n4; i += LP_THREADS) {
            const float4 v = x4[i];
            lp_step4(a, v.x, v.y, v.z, v.w, 4 * i, xt, t);
        }
        const int j = 4 * n4 + tid;                          // the n_vocab % 4 last ids, above every index this thread saw
        if (j < n_vocab) lp_step1(a, x[j], j, xt, t);
    } else {
        for (int j = tid; j < n_vocab; j += LP_THREADS) lp_step1(a, x[j], j, xt, t);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        lp_merge(a, __shfl_xor(a.m, o, 64), __shfl_xor(a.s, o, 64), __shfl_xor(a.c, o, 64), __shfl_xor(a.bi, o, 64));
    __shared__ float sm[LP_THREADS / 64], ss[LP_THREADS / 64];
    __shared__ int sc[LP_THREADS / 64], sb[LP_THREADS / 64];
    const int lane = tid & 63, wid = tid >> 6;
    if (lane == 0) { sm[wid] = a.m; ss[wid] = a.s; sc[wid] = a.c; sb[wid] = a.bi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < LP_THREADS / 64; w++) lp_merge(a, sm[w], ss[w], sc[w], sb[w]);
        lp_out[row] = scored ? (xt - a.m) - logf(a.s) : 0.f;
        if (rank_out) rank_out[row] = scored ? a.c : -1;
        if (argmax_out) argmax_out[row] = (a.bi == 0x7fffffff) ? 0 : a.bi;
    }
}
