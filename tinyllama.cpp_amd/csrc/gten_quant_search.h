// gten_quant_search.h -- include/gten_hip_calib.h's gten_hip_quantize_weight_search: dense f32 / bf16 / f16 weight rows -> packed Q4
// planes whose deltas and quants are chosen per block among 17 candidates by importance-weighted squared error (the header
// states the arithmetic operation by operation; tests/calib_ref.py restates it in NumPy).  Included by gten_ops.hip after
// gten_quant.h, whose loads and scalar steps (load8, absmax_bits8, round_to_src, quant1) it calls and whose candidate-0
// arithmetic and Q4 store it repeats: gten_quant.h stays untouched, so k_quant_pack keeps its instructions.
//
// The ORDER of every sum is part of the definition (a candidate wins by a strict f32 comparison and the test is byte equality),
// so this is VALU arithmetic, not the matrix unit: 17 candidates x 14 f32 operations per element, about 40 x k_quant_pack's
// arithmetic on the same bytes -- the kernel is bound by the VALU, not by HBM.
//
// Work split.  A workgroup (256 threads) owns SR_ROWS = 16 consecutive rows x one group of 512 columns; wave v owns rows
// 4 v .. 4 v + 3 of it and lane l the columns [8 l, 8 l + 8) of the group -- k_quant_pack's layout: quad l / 4 is the block,
// s = l % 4 the eighth of it, which is exactly p_s of the header's sum S.
//     source      the four rows' requests (nontemporal, read once) are issued first; their latency lies under the staging
//     importance  the group's 512 values are shared by all 16 rows: requested once by 128 threads (16 bytes each, checked for a
//                 negative or non-finite value on the way) into two LDS planes Ws[p][lane] of 16 bytes, so a lane's eight
//                 values come back as two ds_read_b128 whose lanes are 16 bytes apart (conflict-free), then live in 8 registers
//     candidates  a lane keeps its 8 elements, 8 weights and the running best (err, f16 delta, candidate number) in registers; a
//                 candidate's quants are 8 more, used twice (A | B, then err) and dropped.  The winner's quants are formed
//                 AGAIN at the end (one division, 8 x mul / rndne / clamp) instead of carrying 8 packed quants through the loop,
//                 which would cost 16 integer operations per candidate under a branch that almost every wave takes
//     S           a lane's 8 terms in ascending order from +0, then two DPP quad steps: + quad_perm[1,0,3,2], + quad_perm[2,3,0,1].
//                 f32 addition commutes, so the four lanes of a quad hold the same bits and decide alike
//     control     no divergent branch: a block that keeps candidate 0 (amax == 0, delta0 zero or not finite), an invalid
//                 candidate and a surplus quad run the same instructions and lose in a select
//     tails       rows % 16: absent rows request nothing and are skipped (wave-uniform);  nb % 16: surplus quads request and store
//                 nothing, as in k_quant_pack
// Plain vector stores only; no packed-f32 instructions; no scratch (tools/kernel_resources.py).
#pragma once

#include <cmath>

#include "gten_quant.h"
#include "../../include/gten_hip_calib.h"

namespace gtq {

constexpr int SR_ROWS = 16;

// the header's S from the four lane sums p_s of a quad: (p_0 + p_1) + (p_2 + p_3), the same bits in all four lanes
__device__ __forceinline__ float quad_tree(float p)
{
    p = p + dpp_mov<0xB1>(p);
    return p + dpp_mov<0x4E>(p);
}

// clamp(rint(x * is), -7, 7) as a float
__device__ __forceinline__ float search_quant(float x, float is)
{
    return fminf(fmaxf(__builtin_rintf(x * is), -7.0f), 7.0f);
}

// err(d, q) of the header
__device__ __forceinline__ float search_err(const float (&x)[8], const float (&w)[8], const float (&q)[8], float d)
{
    float p = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const float e = x[i] - d * q[i];
        p = p + w[i] * (e * e);
    }
    return quad_tree(p);
}

__device__ __forceinline__ bool f16_finite_nonzero(uint16_t h)
{
    return (h & 0x7FFFu) != 0 && (h & 0x7FFFu) < 0x7C00u;
}

// One block of 32 from the eight elements x and weights w each lane of its quad holds (x zeros where !ok).  s = lane % 4;
// b = the block's index in the matrix, nblk their number; every lane of the quad arrives.
template <int SRC>
__device__ __forceinline__ void search_block(const float (&x)[8], const float (&w)[8], bool ok, int s, size_t b, size_t nblk,
                                             uint8_t* __restrict__ dst, unsigned* __restrict__ flags)
{
    // candidate 0: k_quant_pack's amax, delta, scale and quants, statement for statement
    int m = absmax_bits8(x);
    m = nn_max_step<0xB1>(m);
    m = nn_max_step<0x4E>(m);
    if (m >= 0x7F800000 && s == 0) flags[0] = 1u;
    const float amax = __int_as_float(m);
    const float delta = round_to_src<SRC>(amax / 7.0f);
    const float scale = delta != 0.0f ? 1.0f / delta : 0.0f;
    uint16_t dh = f2h(delta);
    const bool search = m > 0 && m < 0x7F800000 && f16_finite_nonzero(dh);

    unsigned p0 = 0, p1 = 0;                                   // quants + 7 of elements 0..3 | 4..7, one byte each
    float q[8];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int lo = quant1(x[i], scale), hi = quant1(x[4 + i], scale);
        p0 |= (unsigned)((lo + 7) & 0xFF) << (8 * i);
        p1 |= (unsigned)((hi + 7) & 0xFF) << (8 * i);
        q[i] = (float)lo;
        q[4 + i] = (float)hi;
    }
    float best = search_err(x, w, q, h2f(dh));
    int bc = 0;

#pragma unroll 1
    for (int c = 1; c <= 16; c++) {
        const float is = (7.0f + 0.125f * (float)(c - 7)) / amax;
        float pa = 0.0f, pb = 0.0f;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            q[i] = search_quant(x[i], is);
            pa = pa + w[i] * (x[i] * q[i]);
            pb = pb + w[i] * (q[i] * q[i]);
        }
        const float A = quad_tree(pa), B = quad_tree(pb);
        const uint16_t h = f2h(A / B);
        const float err = search_err(x, w, q, h2f(h));
        if (search && B > 0.0f && f16_finite_nonzero(h) && err < best) {
            best = err;
            bc = c;
            dh = h;
        }
    }

    // the winner's quants again (quad-uniform select; candidate 0's bytes are already in p0 | p1)
    const float is = (7.0f + 0.125f * (float)(bc - 7)) / amax;
    unsigned w0 = 0, w1 = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        w0 |= (unsigned)((int)search_quant(x[i], is) + 7) << (8 * i);
        w1 |= (unsigned)((int)search_quant(x[4 + i], is) + 7) << (8 * i);
    }
    if (bc) { p0 = w0; p1 = w1; }

    // k_quant_pack's Q4 store: the pair (s, s ^ 2) trades one dword, every lane builds 4 nibble bytes
    const bool low = (s & 2) != 0;                             // this lane holds elements 16..31: the low nibbles
    const unsigned got = (unsigned)dpp_mov_i<0x4E>((int)(low ? p0 : p1));
    const unsigned hi = low ? got : p0, lo = low ? p1 : got;
    if (ok) {
        uint8_t* o = dst + b * 16 + (s & 1) * 8 + (s >> 1) * 4;
        *(unsigned*)o = ((hi << 4) & 0xF0F0F0F0u) | lo;
        if (s == 0) ((uint16_t*)(dst + nblk * 16))[b] = dh;
    }
}

// flags[0]: a source element is not finite;  flags[1]: an importance value is negative or not finite
template <int SRC>
__global__ __launch_bounds__(256) void k_quant_search(const uint8_t* __restrict__ src, const float* __restrict__ importance, uint8_t* __restrict__ dst,
                                                      int rows, int nb, int groups, unsigned* __restrict__ flags)
{
    constexpr int ESZ = src_traits<SRC>::esz;
    __shared__ float4 Ws[2][64];
    const int lane = threadIdx.x & 63, s = lane & 3, wv = threadIdx.x >> 6;
    const size_t row0 = (size_t)(blockIdx.x / (unsigned)groups) * SR_ROWS;           // (the entry point keeps the grid below 2^32)
    const int group = (int)(blockIdx.x % (unsigned)groups);
    const int blk = group * 16 + (lane >> 2);
    const bool col_ok = blk < nb;
    const size_t nblk = (size_t)rows * nb;

    float x[4][8];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const size_t row = row0 + wv * 4 + r;
        const bool ok = col_ok && row < (size_t)rows;
        load8<SRC>(src + ((ok ? row * (size_t)nb + blk : 0) * 32 + s * 8) * ESZ, ok, x[r]);
    }

    if (threadIdx.x < 128) {                                   // thread t: columns 4 t .. 4 t + 3 of the group = half t % 2 of lane t / 2
        const int c = group * 512 + (int)threadIdx.x * 4;
        float4 v = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
        if (importance && c < nb * 32) {                       // (cols % 32 == 0: the four columns exist together)
            v = *(const float4*)(importance + c);
            const bool fine = v.x >= 0.0f && v.x < INFINITY && v.y >= 0.0f && v.y < INFINITY && v.z >= 0.0f && v.z < INFINITY && v.w >= 0.0f && v.w < INFINITY;
            if (!fine) flags[1] = 1u;
        }
        Ws[threadIdx.x & 1][threadIdx.x >> 1] = v;
    }
    __syncthreads();
    const float4 a0 = Ws[0][lane], a1 = Ws[1][lane];
    const float w[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};

#pragma unroll
    for (int r = 0; r < 4; r++) {
        const size_t row = row0 + wv * 4 + r;
        if (row >= (size_t)rows) break;                        // wave-uniform: the quad steps below see whole quads
        search_block<SRC>(x[r], w, col_ok, s, col_ok ? row * (size_t)nb + blk : 0, nblk, dst, flags);
    }
}

static unsigned* g_search_flags = nullptr;   // two device words, zero between calls

} // namespace gtq

extern "C" int gten_hip_quantize_weight_search(const void* src_rows, int src_dtype, int rows, int cols, const float* importance, void* dst_packed)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(src_rows && dst_packed && rows > 0 && cols > 0, "quantize_weight_search: bad arguments");
    GTR_REQUIRE(src_dtype >= GTEN_HIP_SRC_F32 && src_dtype <= GTEN_HIP_SRC_F16, "quantize_weight_search: source dtype %d is not f32, bf16 or f16", src_dtype);
    GTR_REQUIRE(cols % 32 == 0, "quantize_weight_search: cols %d not a multiple of the block size 32", cols);
    GTR_REQUIRE(((uintptr_t)src_rows & 15) == 0 && ((uintptr_t)dst_packed & 15) == 0 && ((uintptr_t)importance & 15) == 0,
                "quantize_weight_search: source, importance and destination must be 16-byte aligned");
    GTR_REQUIRE((size_t)rows * ((cols + 511) / 512) < ((size_t)1 << 32) - 4 && (size_t)rows * cols < ((size_t)1 << 42), "quantize_weight_search: %d x %d is too large for one launch", rows, cols);
    if (!gtq::g_search_flags) {
        GTR_CHECK(hipMalloc((void**)&gtq::g_search_flags, 2 * sizeof(unsigned)));
        GTR_CHECK(hipMemsetAsync(gtq::g_search_flags, 0, 2 * sizeof(unsigned), gtr::stream()));
    }
    gtr::kv_watch_touch(dst_packed, (size_t)rows * gten_hip_row_bytes(GTEN_Q4, cols));
    const uint8_t* s = (const uint8_t*)src_rows;
    const int nb = cols / 32, groups = (cols + 511) / 512;
    const dim3 grid((unsigned)((size_t)((rows + gtq::SR_ROWS - 1) / gtq::SR_ROWS) * groups));
    switch (src_dtype) {
    case GTEN_HIP_SRC_F32: GTR_LAUNCH(KT_PACK, gtq::k_quant_search<GTEN_HIP_SRC_F32>, grid, dim3(256), 0, s, importance, (uint8_t*)dst_packed, rows, nb, groups, gtq::g_search_flags); break;
    case GTEN_HIP_SRC_BF16: GTR_LAUNCH(KT_PACK, gtq::k_quant_search<GTEN_HIP_SRC_BF16>, grid, dim3(256), 0, s, importance, (uint8_t*)dst_packed, rows, nb, groups, gtq::g_search_flags); break;
    default: GTR_LAUNCH(KT_PACK, gtq::k_quant_search<GTEN_HIP_SRC_F16>, grid, dim3(256), 0, s, importance, (uint8_t*)dst_packed, rows, nb, groups, gtq::g_search_flags); break;
    }
    unsigned flags[2] = {0, 0};
    GTR_CHECK(hipMemcpyAsync(flags, gtq::g_search_flags, sizeof(flags), hipMemcpyDeviceToHost, gtr::stream()));
    GTR_CHECK(hipStreamSynchronize(gtr::stream()));
    if (flags[0] | flags[1]) {
        GTR_CHECK(hipMemsetAsync(gtq::g_search_flags, 0, sizeof(flags), gtr::stream()));
        if (flags[0]) return gtr::fail(-4, "quantize_weight_search: the source holds a NaN or an infinity (%d x %d, source dtype %d)", rows, cols, src_dtype);
        return gtr::fail(-4, "quantize_weight_search: the importance holds a negative, NaN or infinite value (%d columns)", cols);
    }
    return 0;
}
