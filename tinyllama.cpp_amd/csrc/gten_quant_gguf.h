// gten_quant_gguf.h -- include/gten_hip_gguf.h: the ggml block stream of a GGUF tensor (Q8_0, Q4_0, Q5_0, Q4_K, Q5_K, Q6_K) decoded
// in registers ON ITS WAY to the packed Q8 / Q4 planes (or f16 rows).  Included by gten_ops.hip after gten_quant_lora.h: the block
// arithmetic behind the decode is that header's pack_block<GTEN_HIP_SRC_F32, WT> (gten_quant.h's absmax_bits8, DPP maxima, quant1,
// plane stores and nibble trade) and its f16_store8 -- called, not repeated.  DESIGN.md 3.29.
//
// The definition D_T (tests/gguf_ref.py restates it in NumPy; d, dmin: f16 widened exactly; (float) of an integer: exact; every
// `*` and `-` one correctly rounded f32 operation, -ffp-contract=off):
//     Q8_0  {f16 d; i8 q[32]}                    x[j]      = (float)q[j] * d
//     Q4_0  {f16 d; u8 qs[16]}                   x[j]      = (float)((qs[j] & 15) - 8) * d
//                                                x[j + 16] = (float)((qs[j] >> 4) - 8) * d
//     Q5_0  {f16 d; u32 qh; u8 qs[16]}           x[j]      = (float)(((qs[j] & 15) | (((qh >> j) & 1) << 4)) - 16) * d
//                                                x[j + 16] = (float)(((qs[j] >> 4) | (((qh >> (j + 16)) & 1) << 4)) - 16) * d
//     Q4_K  {f16 d, dmin; u8 sc[12]; u8 qs[128]}          sub-block j = 2 g + h of 32, element l:  q = (qs[32 g + l] >> 4 h) & 15
//           j < 4:  s = sc[j] & 63                             m = sc[j + 4] & 63
//           else:   s = (sc[j + 4] & 15) | ((sc[j - 4] >> 6) << 4)   m = (sc[j + 4] >> 4) | ((sc[j] >> 6) << 4)
//           t = d * (float)s;   u = t * (float)q;   v = dmin * (float)m;   x = u - v
//     Q5_K  {f16 d, dmin; u8 sc[12]; u8 qh[32]; u8 qs[128]}   as Q4_K with q += 16 * ((qh[l] >> j) & 1)
//     Q6_K  {u8 ql[128]; u8 qh[64]; i8 sc[16]; f16 d}         sub-block j = 4 n + k, element l:
//           q = ((ql[64 n + 32 (k & 1) + l] >> 4 (k >> 1)) & 15) | (((qh[32 n + l] >> 2 k) & 3) << 4)
//           t = d * (float)sc[2 j + l / 16];   x = t * (float)(q - 32)
//
// Work split: k_quant_pack's.  A wave owns 512 consecutive elements of ONE destination row (16 blocks of 32, or 2 super-blocks of
// 256 = 16 sub-blocks); quad l / 4 is the (sub-)block, lane s = l % 4 holds its elements [8 s, 8 s + 8).  What is new is how the eight
// floats reach the lane:
//     row map   the destination row picks its source row in the kernel (n_head > 0: the per-head interleave of attn_q / attn_k
//               undone; include/gten_hip_gguf.h), no index table
//     staging   the wave's bytes -- 16 x {34, 18, 22} or 2 x {144, 176, 210}, at most 544 -- start wherever the row's offset falls
//               (2-byte aligned: row 1 of a 768-column Q6_K matrix is at byte 630).  The wave requests the enclosing 16-byte aligned
//               span, at most 35 slots, with ONE coalesced nontemporal 16-byte request per lane into its own 640 bytes of LDS
//               (the pooling kernels' scheme, DESIGN.md 3.22: a request is issued only where it overlaps a byte that is needed).  4 waves:
//               2560 BYTES OF LDS PER WORKGROUP, one barrier.
//     decode    a lane's 8 quant bytes (and the 8 high-bit bytes of Q5_K / Q6_K, the u32 of Q5_0) are 2-byte aligned in LDS, so they
//               are read as the aligned dwords that cover them and shifted into place by v_alignbyte_b32 (lds_dw / lds_qw): three
//               ds_read_b32 for 8 bytes.  d, dmin: ds_read_u16; the scale bytes: ds_read_u8 / i8, the same address in all four lanes
//               of a quad (a broadcast), unpacked redundantly per lane like k_quant_pack's delta.
//     LDS banks (64 x 4 bytes).  Within a quad the four lanes read consecutive 8-byte pieces: distinct banks, or the SAME dword
//               where a misaligned piece shares one with its neighbour (a broadcast).  Across the 16 quads the pieces lie one
//               block apart (18 / 22 / 34 bytes) or 32 quant bytes apart inside a super-block, the two super-blocks 36 / 44 / 52.5
//               dwords apart.  Counted for each ds_read_b32 over all 64 lanes and every even shift (the most DIFFERENT dwords one
//               bank is asked for): Q4_0 1 (none), Q5_0 2, Q8_0 3 (its 16 blocks span 136 dwords, more than twice the banks),
//               Q4_K 2, Q5_K 2 (qs; qh 1), Q6_K 2 (ql and qh).  So the reads DO collide, two- or three-way; a wave makes three to
//               six such reads per 512 elements, a few LDS cycles beside one HBM round trip.
//     tails     nb % 16 (cols % 512): surplus quads read nothing, hold zeros and store nothing, as in k_quant_pack.
// Plain vector stores only; no packed-f32 instructions; no scratch (tools/kernel_resources.py).
#pragma once

#include "gten_quant_lora.h"
#include "../../include/gten_hip_gguf.h"

namespace gtq {

template <int FMT> struct gguf_traits;      // UNIT: bytes of a block / super-block; ELEMS: its elements
template <> struct gguf_traits<GTEN_GGML_Q8_0> { static constexpr int UNIT = 34, ELEMS = 32; };
template <> struct gguf_traits<GTEN_GGML_Q4_0> { static constexpr int UNIT = 18, ELEMS = 32; };
template <> struct gguf_traits<GTEN_GGML_Q5_0> { static constexpr int UNIT = 22, ELEMS = 32; };
template <> struct gguf_traits<GTEN_GGML_Q4_K> { static constexpr int UNIT = 144, ELEMS = 256; };
template <> struct gguf_traits<GTEN_GGML_Q5_K> { static constexpr int UNIT = 176, ELEMS = 256; };
template <> struct gguf_traits<GTEN_GGML_Q6_K> { static constexpr int UNIT = 210, ELEMS = 256; };

constexpr int GG_WAVE_SLOTS = 40;           // 16-byte slots of LDS per wave: 35 requested at most, the rest is slack for lds_qw's third dword

// the dword / the 8 bytes at byte offset `off` (any alignment) of the LDS words w: the covering aligned dwords, funnel-shifted
__device__ __forceinline__ unsigned lds_dw(const unsigned* w, int off)
{
    const unsigned* p = w + (off >> 2);
    return __builtin_amdgcn_alignbyte(p[1], p[0], (unsigned)off & 3u);
}
__device__ __forceinline__ uint2 lds_qw(const unsigned* w, int off)
{
    const unsigned* p = w + (off >> 2);
    const unsigned a = p[0], b = p[1], c = p[2], sh = (unsigned)off & 3u;
    return make_uint2(__builtin_amdgcn_alignbyte(b, a, sh), __builtin_amdgcn_alignbyte(c, b, sh));
}
__device__ __forceinline__ unsigned byte_of(uint2 v, int i) { return ((i < 4 ? v.x : v.y) >> (8 * (i & 3))) & 0xFFu; }
__device__ __forceinline__ float lds_f16(const unsigned* w, int off)          // off even
{
    float d = h2f(((const uint16_t*)w)[off >> 1]);
    asm("" : "+v"(d));                      // (opaque, like load8's: the widening stays its own instruction)
    return d;
}

// The lane's eight elements of (sub-)block `unit` of the wave's staged bytes.  B: byte offset of the block / super-block in w.
template <int FMT>
__device__ __forceinline__ void gguf_decode8(const unsigned* w, int B, int j, int s, float (&x)[8])
{
    const uint8_t* wb = (const uint8_t*)w;
    if constexpr (FMT == GTEN_GGML_Q8_0) {
        const float d = lds_f16(w, B);
        const uint2 q = lds_qw(w, B + 2 + 8 * s);
#pragma unroll
        for (int i = 0; i < 8; i++) x[i] = (float)(int)(int8_t)byte_of(q, i) * d;
    } else if constexpr (FMT == GTEN_GGML_Q4_0) {
        const float d = lds_f16(w, B);
        const uint2 q = lds_qw(w, B + 2 + 8 * (s & 1));
        const int sh = (s >> 1) * 4;                            // elements 16..31 are the high nibbles
#pragma unroll
        for (int i = 0; i < 8; i++) x[i] = (float)((int)((byte_of(q, i) >> sh) & 15u) - 8) * d;
    } else if constexpr (FMT == GTEN_GGML_Q5_0) {
        const float d = lds_f16(w, B);
        const unsigned qh = lds_dw(w, B + 2) >> (8 * s);        // bit i: the fifth bit of element 8 s + i
        const uint2 q = lds_qw(w, B + 6 + 8 * (s & 1));
        const int sh = (s >> 1) * 4;
#pragma unroll
        for (int i = 0; i < 8; i++) x[i] = (float)((int)(((byte_of(q, i) >> sh) & 15u) | (((qh >> i) & 1u) << 4)) - 16) * d;
    } else if constexpr (FMT == GTEN_GGML_Q4_K || FMT == GTEN_GGML_Q5_K) {
        const float d = lds_f16(w, B), dmin = lds_f16(w, B + 2);
        const uint8_t* sc = wb + B + 4;
        unsigned sv, mv;                                        // the 6-bit scale and min of sub-block j (one address per quad)
        if (j < 4) {
            sv = sc[j] & 63u;
            mv = sc[j + 4] & 63u;
        } else {
            const unsigned hi = sc[j + 4];
            sv = (hi & 15u) | (((unsigned)sc[j - 4] >> 6) << 4);
            mv = (hi >> 4) | (((unsigned)sc[j] >> 6) << 4);
        }
        constexpr int QS = FMT == GTEN_GGML_Q4_K ? 16 : 48;
        const uint2 q = lds_qw(w, B + QS + 32 * (j >> 1) + 8 * s);
        const int sh = (j & 1) * 4;
        uint2 h = make_uint2(0, 0);
        if constexpr (FMT == GTEN_GGML_Q5_K) h = lds_qw(w, B + 16 + 8 * s);
        float t = d * (float)sv, v = dmin * (float)mv;
        asm("" : "+v"(t));
        asm("" : "+v"(v));
#pragma unroll
        for (int i = 0; i < 8; i++) {
            unsigned n = (byte_of(q, i) >> sh) & 15u;
            if constexpr (FMT == GTEN_GGML_Q5_K) n += ((byte_of(h, i) >> j) & 1u) << 4;
            float u = t * (float)n;
            asm("" : "+v"(u));                                  // (opaque: a product, then a difference -- never one fused operation)
            x[i] = u - v;
        }
    } else {
        const int n = j >> 2, k = j & 3;
        const float d = lds_f16(w, B + 208);
        const uint2 ql = lds_qw(w, B + 64 * n + 32 * (k & 1) + 8 * s);
        const uint2 qh = lds_qw(w, B + 128 + 32 * n + 8 * s);
        const int scale = (int)(int8_t)wb[B + 192 + 2 * j + (s >> 1)];
        float t = d * (float)scale;
        asm("" : "+v"(t));
        const int shl = (k >> 1) * 4, shh = 2 * k;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int q = (int)(((byte_of(ql, i) >> shl) & 15u) | (((byte_of(qh, i) >> shh) & 3u) << 4));
            x[i] = t * (float)(q - 32);
        }
    }
#pragma unroll
    for (int i = 0; i < 8; i++) asm("" : "+v"(x[i]));          // (the decoded f32 is a value of its own ahead of the quantiser's multiply)
}

// nb: 32-element blocks of a row; groups: waves of a row; head_rows: rows / n_head, or 0 for the identity row map
template <int FMT, int WT>
__global__ __launch_bounds__(256) void k_quant_gguf(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int rows, int nb, int groups,
                                                    int head_rows, unsigned* __restrict__ nonfinite)
{
    using F = gguf_traits<FMT>;
    constexpr int SUBS = F::ELEMS / 32;                         // 32-element (sub-)blocks of a unit: 1 or 8
    constexpr int UNITS = 16 / SUBS;                            // units of a wave: 16 or 2
    __shared__ uint4 stage[4][GG_WAVE_SLOTS];
    const int lane = threadIdx.x & 63, s = lane & 3, quad = lane >> 2, wv = threadIdx.x >> 6;
    const unsigned wave = blockIdx.x * 4u + (unsigned)wv;       // (the entry point keeps rows * groups below 2^32 - 4)
    const size_t row = wave / (unsigned)groups;
    const int g = (int)(wave % (unsigned)groups);
    const int blk = g * 16 + quad;
    const bool row_ok = row < (size_t)rows;
    const bool ok = row_ok && blk < nb;

    // the source row of this destination row
    size_t srow = row;
    if (head_rows > 0 && row_ok) {
        const unsigned D = (unsigned)head_rows, half = D >> 1, r = (unsigned)row;
        const unsigned h = r / D, rem = r - h * D, t = rem / half, i = rem - t * half;
        srow = (size_t)h * D + 2u * i + t;
    }
    // the wave's units [g * UNITS, ...) of that row: `span` bytes from `begin`, requested as the aligned slots that cover them
    const int units_here = row_ok ? min(UNITS, nb / SUBS - g * UNITS) : 0;
    const size_t begin = srow * (size_t)(nb / SUBS) * F::UNIT + (size_t)g * UNITS * F::UNIT;
    const int shift = (int)(begin & 15), span = units_here * F::UNIT;      // (src is 16-byte aligned: the offset's low bits are the address's)
    if (lane < GG_WAVE_SLOTS) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (span > 0 && lane * 16 < shift + span) v = ld_w16(src + (begin - shift) + (size_t)lane * 16);
        stage[wv][lane] = v;
    }
    __syncthreads();

    float x[8];
#pragma unroll
    for (int i = 0; i < 8; i++) x[i] = 0.0f;
    if (ok) gguf_decode8<FMT>((const unsigned*)stage[wv], shift + (quad / SUBS) * F::UNIT, quad % SUBS, s, x);

    if constexpr (WT == GTEN_F16) {
        if (ok) {
            if (absmax_bits8(x) >= 0x7F800000) *nonfinite = 1u;
            f16_store8(x, (uint16_t*)dst + (row * (size_t)nb + blk) * 32 + s * 8);
        }
    } else {
        pack_block<GTEN_HIP_SRC_F32, WT>(x, ok, s, row, blk, ok ? row * (size_t)nb + blk : 0, nb, (size_t)rows * nb, dst, nonfinite);
    }
}

template <int FMT>
static int launch_gguf(const void* blocks, int rows, int cols, int n_head, int dst_dtype, void* dst)
{
    const int nb = cols / 32, groups = (nb + 15) / 16;
    const unsigned grid = (unsigned)(((size_t)rows * groups + 3) / 4);
    const auto kernel = dst_dtype == GTEN_Q8 ? k_quant_gguf<FMT, GTEN_Q8> : dst_dtype == GTEN_Q4 ? k_quant_gguf<FMT, GTEN_Q4> : k_quant_gguf<FMT, GTEN_F16>;
    GTR_LAUNCH(KT_PACK, kernel, dim3(grid), dim3(256), 0, (const uint8_t*)blocks, (uint8_t*)dst, rows, nb, groups, n_head > 0 ? rows / n_head : 0,
               g_nonfinite);
    return 0;
}

// bytes and elements of a unit of a ggml type; false for a type that is not decoded here
static bool gguf_unit(int ggml_type, int* unit, int* elems)
{
    switch (ggml_type) {
    case GTEN_GGML_Q8_0: *unit = 34; *elems = 32; return true;
    case GTEN_GGML_Q4_0: *unit = 18; *elems = 32; return true;
    case GTEN_GGML_Q5_0: *unit = 22; *elems = 32; return true;
    case GTEN_GGML_Q4_K: *unit = 144; *elems = 256; return true;
    case GTEN_GGML_Q5_K: *unit = 176; *elems = 256; return true;
    case GTEN_GGML_Q6_K: *unit = 210; *elems = 256; return true;
    default: return false;
    }
}

} // namespace gtq

extern "C" size_t gten_hip_gguf_src_bytes(int ggml_type, int rows, int cols)
{
    int unit = 0, elems = 0;
    if (!gtq::gguf_unit(ggml_type, &unit, &elems) || rows <= 0 || cols <= 0 || cols % elems) return 0;
    return (size_t)rows * (size_t)(cols / elems) * (size_t)unit;
}

extern "C" int gten_hip_quantize_weight_gguf(const void* blocks, int ggml_type, int rows, int cols, int n_head, int dst_dtype, void* dst_packed)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(blocks && dst_packed && rows > 0 && cols > 0, "quantize_weight_gguf: bad arguments");
    int unit = 0, elems = 0;
    GTR_REQUIRE(gtq::gguf_unit(ggml_type, &unit, &elems), "quantize_weight_gguf: ggml type %d is not supported (Q4_0 2, Q5_0 6, Q8_0 8, Q4_K 12, Q5_K 13, Q6_K 14)", ggml_type);
    GTR_REQUIRE(cols % elems == 0, "quantize_weight_gguf: cols %d not a multiple of the %d elements of a block of ggml type %d", cols, elems, ggml_type);
    GTR_REQUIRE(dst_dtype == GTEN_Q8 || dst_dtype == GTEN_Q4 || dst_dtype == GTEN_F16, "quantize_weight_gguf: dtype %d is not a weight dtype", dst_dtype);
    GTR_REQUIRE(n_head >= 0 && (n_head == 0 || (rows % n_head == 0 && (rows / n_head) % 2 == 0)),
                "quantize_weight_gguf: n_head %d does not split %d rows into heads of an even number of rows", n_head, rows);
    GTR_REQUIRE(((uintptr_t)blocks & 15) == 0 && ((uintptr_t)dst_packed & 15) == 0, "quantize_weight_gguf: source and destination must be 16-byte aligned");
    GTR_REQUIRE((size_t)rows * ((cols + 511) / 512) < ((size_t)1 << 32) - 4 && (size_t)rows * cols < ((size_t)1 << 42), "quantize_weight_gguf: %d x %d is too large for one launch", rows, cols);
    if (!gtq::g_nonfinite) {
        GTR_CHECK(hipMalloc((void**)&gtq::g_nonfinite, sizeof(unsigned)));
        GTR_CHECK(hipMemsetAsync(gtq::g_nonfinite, 0, sizeof(unsigned), gtr::stream()));
    }
    gtr::kv_watch_touch(dst_packed, (size_t)rows * gten_hip_row_bytes(dst_dtype, cols));
    int rc;
    switch (ggml_type) {
    case GTEN_GGML_Q8_0: rc = gtq::launch_gguf<GTEN_GGML_Q8_0>(blocks, rows, cols, n_head, dst_dtype, dst_packed); break;
    case GTEN_GGML_Q4_0: rc = gtq::launch_gguf<GTEN_GGML_Q4_0>(blocks, rows, cols, n_head, dst_dtype, dst_packed); break;
    case GTEN_GGML_Q5_0: rc = gtq::launch_gguf<GTEN_GGML_Q5_0>(blocks, rows, cols, n_head, dst_dtype, dst_packed); break;
    case GTEN_GGML_Q4_K: rc = gtq::launch_gguf<GTEN_GGML_Q4_K>(blocks, rows, cols, n_head, dst_dtype, dst_packed); break;
    case GTEN_GGML_Q5_K: rc = gtq::launch_gguf<GTEN_GGML_Q5_K>(blocks, rows, cols, n_head, dst_dtype, dst_packed); break;
    default: rc = gtq::launch_gguf<GTEN_GGML_Q6_K>(blocks, rows, cols, n_head, dst_dtype, dst_packed); break;
    }
    if (rc) return rc;
    unsigned flag = 0;
    GTR_CHECK(hipMemcpyAsync(&flag, gtq::g_nonfinite, sizeof(flag), hipMemcpyDeviceToHost, gtr::stream()));
    GTR_CHECK(hipStreamSynchronize(gtr::stream()));
    if (flag) {
        GTR_CHECK(hipMemsetAsync(gtq::g_nonfinite, 0, sizeof(unsigned), gtr::stream()));
        return gtr::fail(-4, "quantize_weight_gguf: a decoded block holds a NaN or an infinity (%d x %d, ggml type %d)", rows, cols, ggml_type);
    }
    return 0;
}
