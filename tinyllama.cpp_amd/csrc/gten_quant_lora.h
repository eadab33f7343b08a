// gten_quant_lora.h -- include/gten_hip_lora.h: a LoRA adapter merged into a dense f32 / bf16 / f16 weight matrix ON ITS WAY to
// the packed Q8 / Q4 planes (or f16 rows): W' = W + scale * B . A formed in registers between gten_quant.h's load and its amax.
// Included by gten_ops.hip after gten_quant.h, whose loads and scalar steps (load8, absmax_bits8, round_to_src, quant1) it calls
// and whose block arithmetic it repeats (pack_block below).
//
// The definition (tests/lora_ref.py restates it in NumPy; every step one correctly rounded f32 operation, no contraction):
//     acc = +0;  for k = 0 .. rank-1 ascending: acc = acc + (B[i][k] * A[k][j]);   m[i][j] = round_to_src(w[i][j] + (scale * acc))
// and the bytes are those of gten_hip_quantize_weight on a source that held m.  The ORDER of the sum is part of the definition
// (quantisation is discontinuous, the test is byte equality), so this is VALU arithmetic and not the matrix unit, whose
// internal accumulation order and fusion cannot be restated.
//
// Work split.  A workgroup (256 threads) owns a tile of LR_ROWS = 16 consecutive rows x one group of 512 columns; wave v owns
// rows 4 v .. 4 v + 3 of it and lane l the columns [8 l, 8 l + 8) of the group -- k_quant_pack's layout (quad l / 4 is the
// block, s = l % 4 the eighth of it), so a lane keeps 4 x 8 accumulators beside its 4 x 8 source elements.
//     source  the four rows' requests (nontemporal, read once) are issued first, so their latency lies under the staging
//     B       the tile's rows, 16 x rank elements, widened and staged ONCE as Bs[k][16 rows]: a wave reads the four values of its
//             rows at rank k with one 16-byte read at a wave-uniform address (a broadcast)
//     A       the group's slice in chunks of LR_CHUNK = 16 ranks, widened while staged: wave v stages ranks v, v + 4, v + 8, v + 12
//             of the chunk, each lane the 8 columns it will later read, as two planes As[p][k][lane] of 16 bytes -- a lane's
//             eight columns come back as two ds_read_b128 whose lanes are 16 bytes apart (conflict-free; [k][512] would put
//             lanes 32 bytes apart, a 2-way conflict).  32 KiB, one buffer, one barrier pair per chunk: rank <= 16, the common
//             adapter, is a single chunk.  A is re-read by every row tile, so its requests keep the default cache policy.
//     k loop  bounded by rank, not padded: 2 LDS reads + 1 broadcast read feed 32 v_mul_f32 + 32 v_add_f32
//     tails   rows % 16: absent rows request nothing, get B = 0 and skip the block arithmetic (wave-uniform);  nb % 16: surplus
//             quads request and store nothing, as in k_quant_pack;  rank % 16: the loop ends at rank
// Plain vector stores only; no packed-f32 instructions; no scratch (tools/kernel_resources.py).
#pragma once

#include <cmath>

#include "gten_quant.h"
#include "../../include/gten_hip_lora.h"

namespace gtq {

constexpr int LR_ROWS = 16, LR_CHUNK = 16, LR_MAX_RANK = GTEN_HIP_LORA_MAX_RANK;

// one A or B element at index i of a dense array -> f32
template <int AB>
__device__ __forceinline__ float widen1(const uint8_t* p, size_t i)
{
    if constexpr (AB == GTEN_HIP_SRC_F32) return __uint_as_float(((const unsigned*)p)[i]);
    else {
        float lo, hi;
        widen2<AB>(((const uint16_t*)p)[i], lo, hi);
        return lo;
    }
}

// elements [0, 8) at p (16-byte aligned) as f32 with the DEFAULT cache policy (A is shared by every row tile)
template <int AB>
__device__ __forceinline__ void load8_keep(const uint8_t* p, bool ok, float4& c0, float4& c1)
{
    uint4 a = make_uint4(0, 0, 0, 0), b = a;
    if constexpr (AB == GTEN_HIP_SRC_F32) {
        if (ok) { a = ld_w16<WLD_KEEP>(p); b = ld_w16<WLD_KEEP>(p + 16); }
        c0 = make_float4(__uint_as_float(a.x), __uint_as_float(a.y), __uint_as_float(a.z), __uint_as_float(a.w));
        c1 = make_float4(__uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z), __uint_as_float(b.w));
    } else {
        if (ok) a = ld_w16<WLD_KEEP>(p);
        widen2<AB>(a.x, c0.x, c0.y);
        widen2<AB>(a.y, c0.z, c0.w);
        widen2<AB>(a.z, c1.x, c1.y);
        widen2<AB>(a.w, c1.z, c1.w);
    }
}

// One block of 32 from the eight elements x each lane of its quad holds (zeros where !ok): k_quant_pack's amax, delta, scale,
// quants and Q8 / Q4 stores, statement for statement.  A COPY, not a shared function: with the tail moved into a function that
// both kernels call, k_quant_pack came out with other registers and another schedule, and that kernel keeps
// its instructions.  s = lane % 4; b = the block's index in the matrix, nblk their number; every lane of the quad arrives.
template <int SRC, int WT>
__device__ __forceinline__ void pack_block(const float (&x)[8], bool ok, int s, size_t row, int blk, size_t b, int nb, size_t nblk,
                                           uint8_t* __restrict__ dst, unsigned* __restrict__ nonfinite)
{
    constexpr float QMAX = WT == GTEN_Q8 ? 127.0f : 7.0f;
    constexpr int BIAS = WT == GTEN_Q8 ? 0 : 7;
    int m = absmax_bits8(x);
    m = nn_max_step<0xB1>(m);
    m = nn_max_step<0x4E>(m);
    if (m >= 0x7F800000 && s == 0) *nonfinite = 1u;
    const float delta = round_to_src<SRC>(__int_as_float(m) / QMAX);
    const float scale = delta != 0.0f ? 1.0f / delta : 0.0f;

    unsigned p0 = 0, p1 = 0;                                   // quants (+ 7 for Q4) of elements 0..3 | 4..7, one byte each
#pragma unroll
    for (int i = 0; i < 4; i++) {
        p0 |= (unsigned)((quant1(x[i], scale) + BIAS) & 0xFF) << (8 * i);
        p1 |= (unsigned)((quant1(x[4 + i], scale) + BIAS) & 0xFF) << (8 * i);
    }

    if constexpr (WT == GTEN_Q8) {
        if (ok) {
            uint8_t* q = dst + row * (size_t)nb * 32 + (size_t)(s >> 1) * nb * 16 + (size_t)blk * 16 + (s & 1) * 8;
            *(uint2*)q = make_uint2(p0, p1);
            if (s == 0) ((uint16_t*)(dst + nblk * 32))[b] = f2h(delta);
        }
    } else {
        const bool low = (s & 2) != 0;                         // this lane holds elements 16..31: the low nibbles
        const unsigned got = (unsigned)dpp_mov_i<0x4E>((int)(low ? p0 : p1));
        const unsigned hi = low ? got : p0, lo = low ? p1 : got;
        if (ok) {
            uint8_t* q = dst + b * 16 + (s & 1) * 8 + (s >> 1) * 4;
            *(unsigned*)q = ((hi << 4) & 0xF0F0F0F0u) | lo;
            if (s == 0) ((uint16_t*)(dst + nblk * 16))[b] = f2h(delta);
        }
    }
}

// eight elements rounded to f16 (nearest even, overflow to infinity) as one 16-byte store
__device__ __forceinline__ void f16_store8(const float (&x)[8], uint16_t* q)
{
    uint4 o;
    o.x = f2h(x[0]) | ((unsigned)f2h(x[1]) << 16);
    o.y = f2h(x[2]) | ((unsigned)f2h(x[3]) << 16);
    o.z = f2h(x[4]) | ((unsigned)f2h(x[5]) << 16);
    o.w = f2h(x[6]) | ((unsigned)f2h(x[7]) << 16);
    *(uint4*)q = o;
}

// The merge of one tile: m[r][0..8) for the wave's four rows at the lane's eight columns.  `x` holds the source elements on
// entry and the merged ones, rounded to the source dtype, on return.  col0: the lane's first column; col_ok: it exists.
template <int SRC, int AB>
__device__ __forceinline__ void merge_tile(float (&x)[4][8], const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, size_t row0, int rows,
                                           size_t cols, size_t col0, bool col_ok, int rank, float scale)
{
    constexpr int AESZ = src_traits<AB>::esz;
    __shared__ float4 As[2][LR_CHUNK][64];
    __shared__ float4 Bs[LR_MAX_RANK][LR_ROWS / 4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;

    // B: element e of the tile's rows x rank block (dense in memory: rows are rank elements apart); absent rows are zeros
    for (int e = threadIdx.x; e < LR_ROWS * rank; e += 256) {
        const int r = e / rank, k = e - r * rank;
        ((float*)Bs)[k * LR_ROWS + r] = row0 + r < (size_t)rows ? widen1<AB>(b, row0 * rank + e) : 0.0f;
    }

    float acc[4][8];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int i = 0; i < 8; i++) acc[r][i] = 0.0f;

    for (int kc = 0; kc < rank; kc += LR_CHUNK) {
        if (kc) __syncthreads();                               // the previous chunk has been read
        float4 c0[4], c1[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int k = kc + wv + 4 * j;
            load8_keep<AB>(a + ((size_t)k * cols + col0) * AESZ, col_ok && k < rank, c0[j], c1[j]);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            As[0][wv + 4 * j][lane] = c0[j];
            As[1][wv + 4 * j][lane] = c1[j];
        }
        __syncthreads();
        const int kn = min(LR_CHUNK, rank - kc);
        for (int k = 0; k < kn; k++) {
            const float4 a0 = As[0][k][lane], a1 = As[1][k][lane], bb = Bs[kc + k][wv];
            const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
            const float bv[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int i = 0; i < 8; i++) acc[r][i] = acc[r][i] + bv[r] * av[i];      // (-ffp-contract=off: a product, then a sum)
        }
    }

#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int i = 0; i < 8; i++) {
            x[r][i] = round_to_src<SRC>(x[r][i] + scale * acc[r][i]);
            asm("" : "+v"(x[r][i]));                           // (opaque, like load8's: the rounding stays its own instruction)
        }
}

template <int SRC, int AB, int WT>
__global__ __launch_bounds__(256) void k_quant_pack_lora(const uint8_t* __restrict__ src, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                         uint8_t* __restrict__ dst, int rows, int nb, int groups, int rank, float scale,
                                                         unsigned* __restrict__ nonfinite)
{
    constexpr int ESZ = src_traits<SRC>::esz;
    const int lane = threadIdx.x & 63, s = lane & 3, wv = threadIdx.x >> 6;
    const size_t row0 = (size_t)(blockIdx.x / (unsigned)groups) * LR_ROWS;           // (the entry point keeps the grid below 2^32)
    const int blk = (int)(blockIdx.x % (unsigned)groups) * 16 + (lane >> 2);
    const bool col_ok = blk < nb;
    const size_t nblk = (size_t)rows * nb;

    float x[4][8];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const size_t row = row0 + wv * 4 + r;
        const bool ok = col_ok && row < (size_t)rows;
        load8<SRC>(src + ((ok ? row * (size_t)nb + blk : 0) * 32 + s * 8) * ESZ, ok, x[r]);
    }
    merge_tile<SRC, AB>(x, a, b, row0, rows, (size_t)nb * 32, (size_t)blk * 32 + s * 8, col_ok, rank, scale);
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const size_t row = row0 + wv * 4 + r;
        if (row >= (size_t)rows) break;                        // wave-uniform: the quad steps below see whole quads
        if (!col_ok)
#pragma unroll
            for (int i = 0; i < 8; i++) x[r][i] = 0.0f;
        pack_block<SRC, WT>(x[r], col_ok, s, row, blk, col_ok ? row * (size_t)nb + blk : 0, nb, nblk, dst, nonfinite);
    }
}

// f16 destination: the same tile; cols % 8 == 0, so a lane's eight columns exist together and leave as one 16-byte store
template <int SRC, int AB>
__global__ __launch_bounds__(256) void k_quant_f16_lora(const uint8_t* __restrict__ src, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                        uint16_t* __restrict__ dst, int rows, int cols, int groups, int rank, float scale,
                                                        unsigned* __restrict__ nonfinite)
{
    constexpr int ESZ = src_traits<SRC>::esz;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t row0 = (size_t)(blockIdx.x / (unsigned)groups) * LR_ROWS;
    const size_t col0 = (size_t)(blockIdx.x % (unsigned)groups) * 512 + lane * 8;
    const bool col_ok = col0 < (size_t)cols;

    float x[4][8];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const size_t row = row0 + wv * 4 + r;
        const bool ok = col_ok && row < (size_t)rows;
        load8<SRC>(src + (ok ? row * (size_t)cols + col0 : 0) * ESZ, ok, x[r]);
    }
    merge_tile<SRC, AB>(x, a, b, row0, rows, (size_t)cols, col0, col_ok, rank, scale);
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const size_t row = row0 + wv * 4 + r;
        if (!col_ok || row >= (size_t)rows) continue;
        if (absmax_bits8(x[r]) >= 0x7F800000) *nonfinite = 1u;
        f16_store8(x[r], dst + row * (size_t)cols + col0);
    }
}

template <int SRC, int AB>
static int launch_lora(const void* src, int rows, int cols, const void* a, const void* b, int rank, float scale, int dst_dtype, void* dst)
{
    const uint8_t *s = (const uint8_t*)src, *pa = (const uint8_t*)a, *pb = (const uint8_t*)b;
    const int groups = (cols + 511) / 512;
    const dim3 grid((unsigned)((size_t)((rows + LR_ROWS - 1) / LR_ROWS) * groups));
    if (dst_dtype == GTEN_F16) {
        GTR_LAUNCH(KT_PACK, (k_quant_f16_lora<SRC, AB>), grid, dim3(256), 0, s, pa, pb, (uint16_t*)dst, rows, cols, groups, rank, scale, g_nonfinite);
        return 0;
    }
    const auto kernel = dst_dtype == GTEN_Q8 ? k_quant_pack_lora<SRC, AB, GTEN_Q8> : k_quant_pack_lora<SRC, AB, GTEN_Q4>;
    GTR_LAUNCH(KT_PACK, kernel, grid, dim3(256), 0, s, pa, pb, (uint8_t*)dst, rows, cols / 32, groups, rank, scale, g_nonfinite);
    return 0;
}

template <int SRC>
static int launch_lora_ab(int ab_dtype, const void* src, int rows, int cols, const void* a, const void* b, int rank, float scale, int dst_dtype, void* dst)
{
    switch (ab_dtype) {
    case GTEN_HIP_SRC_F32: return launch_lora<SRC, GTEN_HIP_SRC_F32>(src, rows, cols, a, b, rank, scale, dst_dtype, dst);
    case GTEN_HIP_SRC_BF16: return launch_lora<SRC, GTEN_HIP_SRC_BF16>(src, rows, cols, a, b, rank, scale, dst_dtype, dst);
    default: return launch_lora<SRC, GTEN_HIP_SRC_F16>(src, rows, cols, a, b, rank, scale, dst_dtype, dst);
    }
}

} // namespace gtq

extern "C" int gten_hip_quantize_weight_lora(const void* src_rows, int src_dtype, int rows, int cols, const void* a, const void* b, int rank,
                                             int ab_dtype, float scale, int dst_dtype, void* dst_packed)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(src_rows && dst_packed && a && b && rows > 0 && cols > 0, "quantize_weight_lora: bad arguments");
    GTR_REQUIRE(src_dtype >= GTEN_HIP_SRC_F32 && src_dtype <= GTEN_HIP_SRC_F16, "quantize_weight_lora: source dtype %d is not f32, bf16 or f16", src_dtype);
    GTR_REQUIRE(ab_dtype >= GTEN_HIP_SRC_F32 && ab_dtype <= GTEN_HIP_SRC_F16, "quantize_weight_lora: adapter dtype %d is not f32, bf16 or f16", ab_dtype);
    GTR_REQUIRE(rank >= 1 && rank <= gtq::LR_MAX_RANK, "quantize_weight_lora: rank %d is outside 1..%d", rank, gtq::LR_MAX_RANK);
    GTR_REQUIRE(std::isfinite(scale), "quantize_weight_lora: the scale is not finite");
    GTR_REQUIRE(dst_dtype == GTEN_Q8 || dst_dtype == GTEN_Q4 || dst_dtype == GTEN_F16, "quantize_weight_lora: dtype %d is not a weight dtype", dst_dtype);
    GTR_REQUIRE(dst_dtype == GTEN_F16 || cols % 32 == 0, "quantize_weight_lora: cols %d not a multiple of the block size 32", cols);
    GTR_REQUIRE(cols % 8 == 0, "quantize_weight_lora: cols %d not a multiple of 8 (the rows of A must keep the base's 16-byte alignment)", cols);
    GTR_REQUIRE(((uintptr_t)src_rows & 15) == 0 && ((uintptr_t)dst_packed & 15) == 0, "quantize_weight_lora: source and destination must be 16-byte aligned");
    GTR_REQUIRE(((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0, "quantize_weight_lora: A and B must be 16-byte aligned");
    GTR_REQUIRE((size_t)rows * ((cols + 511) / 512) < ((size_t)1 << 32) - 4 && (size_t)rows * cols < ((size_t)1 << 42), "quantize_weight_lora: %d x %d is too large for one launch", rows, cols);
    if (!gtq::g_nonfinite) {
        GTR_CHECK(hipMalloc((void**)&gtq::g_nonfinite, sizeof(unsigned)));
        GTR_CHECK(hipMemsetAsync(gtq::g_nonfinite, 0, sizeof(unsigned), gtr::stream()));
    }
    gtr::kv_watch_touch(dst_packed, (size_t)rows * gten_hip_row_bytes(dst_dtype, cols));
    int rc;
    switch (src_dtype) {
    case GTEN_HIP_SRC_F32: rc = gtq::launch_lora_ab<GTEN_HIP_SRC_F32>(ab_dtype, src_rows, rows, cols, a, b, rank, scale, dst_dtype, dst_packed); break;
    case GTEN_HIP_SRC_BF16: rc = gtq::launch_lora_ab<GTEN_HIP_SRC_BF16>(ab_dtype, src_rows, rows, cols, a, b, rank, scale, dst_dtype, dst_packed); break;
    default: rc = gtq::launch_lora_ab<GTEN_HIP_SRC_F16>(ab_dtype, src_rows, rows, cols, a, b, rank, scale, dst_dtype, dst_packed); break;
    }
    if (rc) return rc;
    unsigned flag = 0;
    GTR_CHECK(hipMemcpyAsync(&flag, gtq::g_nonfinite, sizeof(flag), hipMemcpyDeviceToHost, gtr::stream()));
    GTR_CHECK(hipStreamSynchronize(gtr::stream()));
    if (flag) {
        GTR_CHECK(hipMemsetAsync(gtq::g_nonfinite, 0, sizeof(unsigned), gtr::stream()));
        return gtr::fail(-4, "quantize_weight_lora: the merged matrix holds a NaN or an infinity (%d x %d, rank %d, source dtype %d, adapter dtype %d)",
                         rows, cols, rank, src_dtype, ab_dtype);
    }
    return 0;
}
