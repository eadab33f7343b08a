// gten_quant.h -- include/gten_hip_quant.h: dense f32 / bf16 / f16 weight rows -> the packed Q8 / Q4 planes (or f16 rows) the
// operators read, quantised on the device in one launch.  Included by gten_ops.hip.
//
// The arithmetic is tinyllama.cpp_amd/convert.py:60-92, operation by operation (every step is one correctly rounded IEEE
// operation in both places, so the bytes are equal, not close):
//     amax / qmax         the compiler's IEEE f32 division (correctly rounded, denormals kept)
//     round_to_src        bf16: the converter's integer rounding of the upper 16 bits;  f16: v_cvt_f16_f32 and back
//     1.0f / delta32      IEEE division again;  0 for a zero delta
//     rint(x * scale)     v_mul_f32, v_rndne_f32 (no contraction: -ffp-contract=off), then NumPy-on-x86's int32 conversion
//                         (out of range or NaN -> INT_MIN; reachable only through an infinite scale, f32 denormal deltas)
//
// Work split (k_quant_pack).  One wave owns 16 consecutive blocks of one row = 512 elements: one 1 KiB request for 16-bit
// sources, two for f32.  Lane l belongs to quad l / 4 = the block, and holds elements [8 s, 8 s + 8) of it, s = l % 4:
//     amax     8 integer maxima of |x| bit patterns per lane (non-negative floats order like their bits; a NaN or an infinity
//              is the largest pattern, so the same maximum finds non-finite input), then two DPP quad steps
//     delta, scale   redundantly in the four lanes of the quad
//     quants   eight per lane, kept as the low bytes of two dwords
//     Q8       lanes s = 0, 1 store their 8 bytes into half-block plane 0, s = 2, 3 into plane 1 (global_store_dwordx2)
//     Q4       byte j needs element j (lanes s = 0, 1) and element j + 16 (lanes s = 2, 3): the pair (s, s ^ 2) trades ONE dword
//              through quad_perm[2,3,0,1] -- s < 2 sends its elements 4..7 and keeps 0..3, s >= 2 the other way round -- so
//              every lane builds 4 nibble bytes and the wave writes its 256 contiguous bytes with one global_store_dword
//     delta    lane s = 0 of each quad stores the f16
// No LDS, no barrier, 8 live floats per lane.  The source is read once: nontemporal loads.  A row whose nb is not a multiple
// of 16 ends in a group whose surplus quads load nothing (zeros) and store nothing.
#pragma once

#include "gten_dev.h"
#include "gten_rt.h"
#include "../../include/gten_hip_quant.h"

namespace gtq {

using namespace gtd;

template <int SRC> struct src_traits { static constexpr int esz = 2; };
template <> struct src_traits<GTEN_HIP_SRC_F32> { static constexpr int esz = 4; };

// two 16-bit source elements of one dword -> f32
template <int SRC>
__device__ __forceinline__ void widen2(unsigned w, float& lo, float& hi)
{
    if constexpr (SRC == GTEN_HIP_SRC_BF16) {
        lo = __uint_as_float(w << 16);
        hi = __uint_as_float(w & 0xFFFF0000u);
    } else {
        lo = h2f((uint16_t)(w & 0xFFFFu));
        hi = h2f((uint16_t)(w >> 16));
    }
}

// elements [0, 8) at p (16-byte aligned) as f32; nothing is requested when !ok
template <int SRC>
__device__ __forceinline__ void load8(const uint8_t* p, bool ok, float (&x)[8])
{
    if constexpr (SRC == GTEN_HIP_SRC_F32) {
        uint4 a = make_uint4(0, 0, 0, 0), b = a;
        if (ok) { a = ld_w16(p); b = ld_w16(p + 16); }
        x[0] = __uint_as_float(a.x); x[1] = __uint_as_float(a.y); x[2] = __uint_as_float(a.z); x[3] = __uint_as_float(a.w);
        x[4] = __uint_as_float(b.x); x[5] = __uint_as_float(b.y); x[6] = __uint_as_float(b.z); x[7] = __uint_as_float(b.w);
    } else {
        uint4 a = make_uint4(0, 0, 0, 0);
        if (ok) a = ld_w16(p);
        widen2<SRC>(a.x, x[0], x[1]);
        widen2<SRC>(a.y, x[2], x[3]);
        widen2<SRC>(a.z, x[4], x[5]);
        widen2<SRC>(a.w, x[6], x[7]);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) asm("" : "+v"(x[i]));      // (opaque: the widening stays its own instruction, no mixed-precision multiply)
}

// max over the |x| bit patterns of a lane's elements: >= 0x7F800000 exactly when one of them is not finite
__device__ __forceinline__ int absmax_bits8(const float (&x)[8])
{
    int m = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) m = max(m, __float_as_int(x[i]) & 0x7FFFFFFF);
    return m;
}

// convert.py:_round_to
template <int SRC>
__device__ __forceinline__ float round_to_src(float v)
{
    if constexpr (SRC == GTEN_HIP_SRC_BF16) {
        const unsigned u = __float_as_uint(v);
        return __uint_as_float((u + 0x7FFFu + ((u >> 16) & 1u)) & 0xFFFF0000u);
    } else if constexpr (SRC == GTEN_HIP_SRC_F16) {
        return (float)f2hv(v);
    } else {
        return v;
    }
}

// np.rint(x * scale).astype(np.int32) on x86: values outside int32 (and NaN) become INT_MIN
__device__ __forceinline__ int quant1(float x, float scale)
{
    const float r = __builtin_rintf(x * scale);
    return (__builtin_fabsf(r) < 2147483648.0f) ? (int)r : (int)0x80000000;
}

template <int SRC, int WT>
__global__ __launch_bounds__(256) void k_quant_pack(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int rows, int nb, int groups,
                                                    unsigned* __restrict__ nonfinite)
{
    constexpr int ESZ = src_traits<SRC>::esz;
    constexpr float QMAX = WT == GTEN_Q8 ? 127.0f : 7.0f;
    constexpr int BIAS = WT == GTEN_Q8 ? 0 : 7;
    const int lane = threadIdx.x & 63, s = lane & 3;
    const unsigned wave = blockIdx.x * 4u + (threadIdx.x >> 6);       // (the entry point keeps rows * groups below 2^32 - 4)
    const size_t row = wave / (unsigned)groups;
    const int blk = (int)(wave % (unsigned)groups) * 16 + (lane >> 2);
    const bool ok = row < (size_t)rows && blk < nb;
    const size_t b = ok ? row * (size_t)nb + blk : 0;          // the block's index in the matrix
    const size_t nblk = (size_t)rows * nb;

    float x[8];
    load8<SRC>(src + (b * 32 + s * 8) * ESZ, ok, x);

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
            // bytes [0,4) from s = 0, [4,8) from s = 2, [8,12) from s = 1, [12,16) from s = 3
            uint8_t* q = dst + b * 16 + (s & 1) * 8 + (s >> 1) * 4;
            *(unsigned*)q = ((hi << 4) & 0xF0F0F0F0u) | lo;
            if (s == 0) ((uint16_t*)(dst + nblk * 16))[b] = f2h(delta);
        }
    }
}

// f16 destination: the matrix as n flat elements, 8 per lane; the last lane takes the tail element by element
template <int SRC>
__global__ __launch_bounds__(256) void k_quant_f16(const uint8_t* __restrict__ src, uint16_t* __restrict__ dst, size_t n, unsigned* __restrict__ nonfinite)
{
    constexpr int ESZ = src_traits<SRC>::esz;
    const size_t e = ((size_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (e >= n) return;
    const bool full = e + 8 <= n;
    float x[8];
    load8<SRC>(src + e * ESZ, full, x);
    if (!full) {
        for (size_t i = e; i < n; i++) {
            float lo, hi;
            if constexpr (SRC == GTEN_HIP_SRC_F32) lo = __uint_as_float(*(const unsigned*)(src + i * 4));
            else widen2<SRC>(*(const uint16_t*)(src + i * 2), lo, hi);
            x[i - e] = lo;
        }
    }
    if (absmax_bits8(x) >= 0x7F800000) *nonfinite = 1u;
    if (full) {
        uint4 o;
        o.x = f2h(x[0]) | ((unsigned)f2h(x[1]) << 16);
        o.y = f2h(x[2]) | ((unsigned)f2h(x[3]) << 16);
        o.z = f2h(x[4]) | ((unsigned)f2h(x[5]) << 16);
        o.w = f2h(x[6]) | ((unsigned)f2h(x[7]) << 16);
        *(uint4*)(dst + e) = o;
    } else {
#pragma unroll
        for (int i = 0; i < 8; i++)
            if (e + i < n) dst[e + i] = f2h(x[i]);
    }
}

static unsigned* g_nonfinite = nullptr;      // one device word, zero between calls

template <int SRC>
static int launch(const void* src, int rows, int cols, int dst_dtype, void* dst)
{
    const uint8_t* s = (const uint8_t*)src;
    if (dst_dtype == GTEN_F16) {
        const size_t n = (size_t)rows * cols;
        GTR_LAUNCH(KT_PACK, k_quant_f16<SRC>, dim3((unsigned)((n + 2047) / 2048)), dim3(256), 0, s, (uint16_t*)dst, n, g_nonfinite);
        return 0;
    }
    const int nb = cols / 32, groups = (nb + 15) / 16;
    const unsigned grid = (unsigned)(((size_t)rows * groups + 3) / 4);
    const auto kernel = dst_dtype == GTEN_Q8 ? k_quant_pack<SRC, GTEN_Q8> : k_quant_pack<SRC, GTEN_Q4>;
    GTR_LAUNCH(KT_PACK, kernel, dim3(grid), dim3(256), 0, s, (uint8_t*)dst, rows, nb, groups, g_nonfinite);
    return 0;
}

} // namespace gtq

extern "C" size_t gten_hip_quant_src_bytes(int src_dtype, int rows, int cols)
{
    if (src_dtype < GTEN_HIP_SRC_F32 || src_dtype > GTEN_HIP_SRC_F16 || rows <= 0 || cols <= 0) return 0;
    return (size_t)rows * (size_t)cols * (src_dtype == GTEN_HIP_SRC_F32 ? 4 : 2);
}

extern "C" int gten_hip_quantize_weight(const void* src_rows, int src_dtype, int rows, int cols, int dst_dtype, void* dst_packed)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(src_rows && dst_packed && rows > 0 && cols > 0, "quantize_weight: bad arguments");
    GTR_REQUIRE(src_dtype >= GTEN_HIP_SRC_F32 && src_dtype <= GTEN_HIP_SRC_F16, "quantize_weight: source dtype %d is not f32, bf16 or f16", src_dtype);
    GTR_REQUIRE(dst_dtype == GTEN_Q8 || dst_dtype == GTEN_Q4 || dst_dtype == GTEN_F16, "quantize_weight: dtype %d is not a weight dtype", dst_dtype);
    GTR_REQUIRE(dst_dtype == GTEN_F16 || cols % 32 == 0, "quantize_weight: cols %d not a multiple of the block size 32", cols);
    GTR_REQUIRE(((uintptr_t)src_rows & 15) == 0 && ((uintptr_t)dst_packed & 15) == 0, "quantize_weight: source and destination must be 16-byte aligned");
    GTR_REQUIRE((size_t)rows * ((cols + 511) / 512) < ((size_t)1 << 32) - 4 && (size_t)rows * cols < ((size_t)1 << 42), "quantize_weight: %d x %d is too large for one launch", rows, cols);
    if (!gtq::g_nonfinite) {
        GTR_CHECK(hipMalloc((void**)&gtq::g_nonfinite, sizeof(unsigned)));
        GTR_CHECK(hipMemsetAsync(gtq::g_nonfinite, 0, sizeof(unsigned), gtr::stream()));
    }
    gtr::kv_watch_touch(dst_packed, (size_t)rows * gten_hip_row_bytes(dst_dtype, cols));
    int rc;
    switch (src_dtype) {
    case GTEN_HIP_SRC_F32: rc = gtq::launch<GTEN_HIP_SRC_F32>(src_rows, rows, cols, dst_dtype, dst_packed); break;
    case GTEN_HIP_SRC_BF16: rc = gtq::launch<GTEN_HIP_SRC_BF16>(src_rows, rows, cols, dst_dtype, dst_packed); break;
    default: rc = gtq::launch<GTEN_HIP_SRC_F16>(src_rows, rows, cols, dst_dtype, dst_packed); break;
    }
    if (rc) return rc;
    unsigned flag = 0;
    GTR_CHECK(hipMemcpyAsync(&flag, gtq::g_nonfinite, sizeof(flag), hipMemcpyDeviceToHost, gtr::stream()));
    GTR_CHECK(hipStreamSynchronize(gtr::stream()));
    if (flag) {
        GTR_CHECK(hipMemsetAsync(gtq::g_nonfinite, 0, sizeof(unsigned), gtr::stream()));
        return gtr::fail(-4, "quantize_weight: the source holds a NaN or an infinity (%d x %d, source dtype %d)", rows, cols, src_dtype);
    }
    return 0;
}
