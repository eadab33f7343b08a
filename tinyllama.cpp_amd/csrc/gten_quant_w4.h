// gten_quant_w4.h -- include/gten_hip_w4.h: the qweight / qzeros / scales (/ g_idx) tensors of a GPTQ or AWQ 4-bit checkpoint unpacked,
// TRANSPOSED and dequantised ON THEIR WAY to the packed Q8 / Q4 planes (or f16 rows).  Included by gten_ops.hip after gten_quant_gguf.h.
// The block arithmetic behind the decode is gten_quant_lora.h's pack_block<GTEN_HIP_SRC_F16, WT> and f16_store8 -- called, not
// repeated: they work per quad, so a wave's 16 quads may hold any 16 blocks.  DESIGN.md 3.30.
//
// The definition (tests/w4_ref.py restates it in NumPy).  Our weight is [N out][K in]; G groups; P = {0, 4, 1, 5, 2, 6, 3, 7}:
//     GPTQ  qweight [K/8][N]   q(k, n) = (qweight[k >> 3][n] >> 4 (k & 7)) & 15        z(g, n) = ((qzeros[g][n >> 3] >> 4 (n & 7)) & 15) + zero_offset
//     AWQ   qweight [K][N/8]   q(k, n) = (qweight[k][n >> 3] >> 4 P[n & 7]) & 15       z(g, n) = (qzeros[g][n >> 3] >> 4 P[n & 7]) & 15
//     g(k) = g_idx ? g_idx[k] : k / group_size        D(n, k) = to_f16((float)(q - z) * widen(scales[g][n]))
// The product of an f16 and an integer in [-16, 15] is exact in f32: one v_mul_f32, one v_cvt_f16_f32 (-ffp-contract=off).
//
// Every format the other quantising kernels read is row-major: a destination block's 32 elements are contiguous in the source.
// Here they lie 4 words that are 4 N bytes apart (GPTQ), or one nibble in each of 32 words (AWQ).  So the split is a TILE, not a row:
//     tile      a workgroup (256 threads) owns W4_TK = 256 input columns (8 blocks of a row: 128 contiguous bytes of a Q4 row, 2 x 128
//               of the two Q8 planes, 512 of an f16 row) x TN output rows.  blockIdx.x runs along K first, so workgroups in flight
//               together write neighbouring runs of the same destination rows.
//               GPTQ  TN = 64:  32 word-rows of 64 words, every request run 256 contiguous bytes along N.   8 KiB packed.
//               AWQ   TN = 256: 256 rows of 32 words, every run 128 bytes.                                 32 KiB packed.
//     requests  the words are read ONCE, nontemporally, as 16-byte requests (2 per thread GPTQ, 8 AWQ, all issued before the first
//               LDS write).  An AWQ row is N / 2 bytes, 16-byte aligned only when N % 32 == 0: other N take the same loop with
//               4-byte requests (32 per thread; the slow, correct form for odd shapes).  The tile stays 4 bits wide in LDS.
//     LDS       GPTQ  qw[32][65] words.  Lane s of block (n, b) needs k = 32 b + 8 s .. + 7 of column n: exactly ONE word,
//               [4 b + s][n] -- one ds_read_b32, eight shifts.  A wave takes two columns 32 apart (nl, nl + 32) x the tile's 8
//               blocks: quads 0-7 read the 32 word-rows of column nl, quads 8-15 those of nl + 32.  With the odd pitch 65 the bank
//               is (r + nl) % 64 and (r + nl + 32) % 64 for r = 0..31: 64 lanes on 64 distinct banks, no collision (and none in
//               either half of the wave on 32 banks).  The pitch is odd, so the staging stores are ds_write_b32: lane (r, c) of a
//               wave stores words 4 c + i of rows r .. r + 3 -- bank (r + 4 c + i) % 64, distinct.
//               AWQ   qw[256][33] words.  The same eight elements are one nibble of each of EIGHT words, [32 b + 8 s + i][n >> 3] at
//               position P[n & 7].  A wave takes the eight columns of ONE word column c in quads 0-7 and again in quads 8-15 for
//               the next block: the eight quads read the SAME word (a broadcast) and shift by their own P[j].  Per ds_read_b32
//               the wave asks for 8 different words, rows 8 apart: banks (8 m * 33 + c) % 64 = (8 m + c) % 64, m = 0..7, distinct.
//               Eight reads per block against GPTQ's one: counted, not removed.  Its staging stores (ds_write_b32, pitch 33) DO
//               collide two-way: rows r and r + 4 of one wave's requests meet on a bank; 32 stores per thread beside 256 reads.
//     tables    without g_idx a block lies in ONE group: a tile touches at most W4_MAXG = 8 (group_size >= 32).  Their scales rows
//               (TN f16 each, 16-byte requests, default cache policy: K tiles of one group re-read them) and qzeros words are
//               staged once: sc[8][TN] f16 + zw[8][TN / 8] words = 1.25 KiB (GPTQ) / 5 KiB (AWQ).  One ds_read_u16 + one
//               ds_read_b32 per block, the same address in the four lanes of a quad.  Across a GPTQ wave's quads the scale
//               reads lie g * 32 + n / 2 words apart: no collision for group_size >= 128 (two groups a tile), 2-way at 64, 4-way at
//               32 -- one read per block, not padded away.
//               with g_idx (template ACT, GPTQ only) the group is PER ELEMENT: g_idx[k0 .. k0 + 256) is staged (1 KiB), each entry
//               CHECKED against [0, G) there -- a bad one raises flags[1] and is replaced by 0, so no address is ever formed from
//               it -- and scales[g][n] / the zero word are fetched per element through L2.  The slow, correct form.
//     passes    GPTQ: 8 passes of 64 quads (b = quad % 8 stays, so the block's group is found once); AWQ: 8 word columns per wave x
//               4 block pairs.  8 live floats per lane, as in k_quant_pack.
//     tails     N % TN, K % 256: absent words are not requested; surplus quads read nothing, hold zeros and store nothing.
// Plain vector stores only; no packed-f32 instructions; no scratch (tools/kernel_resources.py).
#pragma once

#include "gten_quant_gguf.h"
#include "../../include/gten_hip_w4.h"

namespace gtq {

constexpr int W4_TK = 256;                  // input columns of a tile
constexpr int W4_MAXG = 8;                  // groups a tile can touch without g_idx: group_size >= 32, group starts are multiples of 32

// TN: output rows of a tile; SRC_ROWS x ROW_WORDS: its qweight words; PITCH: words between its rows in LDS
template <int LAYOUT> struct w4_traits;
template <> struct w4_traits<GTEN_W4_GPTQ> { static constexpr int TN = 64, SRC_ROWS = W4_TK / 8, ROW_WORDS = 64, PITCH = 65; };
template <> struct w4_traits<GTEN_W4_AWQ> { static constexpr int TN = 256, SRC_ROWS = W4_TK, ROW_WORDS = 32, PITCH = 33; };

__device__ __forceinline__ float w4_widen(uint16_t h)
{
    float d = h2f(h);
    asm("" : "+v"(d));                      // (opaque, like load8's: the widening stays its own instruction)
    return d;
}
// D for one element: the f32 product, rounded to f16 (f2hv makes the product a value of its own first), widened again
__device__ __forceinline__ float w4_value(unsigned q, int z, float scale)
{
    return (float)f2hv((float)((int)q - z) * scale);
}

// the block's eight elements in the lane -> the destination (every lane of the quad arrives: pack_block trades through DPP)
template <int WT>
__device__ __forceinline__ void w4_emit(float (&x)[8], bool ok, int s, int n, int blk, int N, int nb, uint8_t* __restrict__ dst, unsigned* __restrict__ flags)
{
#pragma unroll
    for (int i = 0; i < 8; i++) asm("" : "+v"(x[i]));          // (D is a value of its own ahead of the quantiser's multiply)
    if constexpr (WT == GTEN_F16) {
        if (ok) {
            if (absmax_bits8(x) >= 0x7F800000) flags[0] = 1u;
            f16_store8(x, (uint16_t*)dst + ((size_t)n * nb + blk) * 32 + s * 8);
        }
    } else {
        pack_block<GTEN_HIP_SRC_F16, WT>(x, ok, s, (size_t)n, blk, ok ? (size_t)n * nb + blk : 0, nb, (size_t)N * nb, dst, flags);
    }
}

// gs: the group size (K for one group); G: groups; tiles_k: tiles along K; flags: [0] a non-finite D, [1] a g_idx entry outside [0, G)
template <int LAYOUT, bool ACT, int WT>
__global__ __launch_bounds__(256) void k_quant_w4(const unsigned* __restrict__ qweight, const unsigned* __restrict__ qzeros,
                                                  const uint16_t* __restrict__ scales, const int* __restrict__ g_idx, uint8_t* __restrict__ dst,
                                                  int N, int K, int gs, int G, int zoff, int tiles_k, unsigned* __restrict__ flags)
{
    using T = w4_traits<LAYOUT>;
    constexpr int TN = T::TN, PITCH = T::PITCH, TW = TN / 8;
    static_assert(!ACT || LAYOUT == GTEN_W4_GPTQ, "only GPTQ has a g_idx");
    __shared__ unsigned qw[T::SRC_ROWS * PITCH];
    __shared__ uint4 sc4[ACT ? 1 : W4_MAXG * TW];               // sc[gl][TN] f16
    __shared__ unsigned zw[ACT ? 1 : W4_MAXG * TW];             // zw[gl][TN / 8]
    __shared__ int gi[ACT ? W4_TK : 1];
    const uint16_t* sc = (const uint16_t*)sc4;

    const int tid = threadIdx.x, lane = tid & 63, s = lane & 3, quad = lane >> 2, wv = tid >> 6;
    const int kt = (int)(blockIdx.x % (unsigned)tiles_k), nt = (int)(blockIdx.x / (unsigned)tiles_k);
    const int n0 = nt * TN, k0 = kt * W4_TK, kb0 = kt * (W4_TK / 32), nb = K / 32, nw = N / 8;

    // ---- the tile's packed words, as they lie: rows of the SOURCE (word-rows of 8 k for GPTQ, single k for AWQ), columns along N
    constexpr bool GP = LAYOUT == GTEN_W4_GPTQ;
    const int src_rows = GP ? K / 8 : K, src_cols = GP ? N : nw;
    const int r0 = GP ? k0 / 8 : k0, c0 = GP ? n0 : n0 / 8;
    if (GP || (src_cols & 3) == 0) {
        constexpr int RQ = T::ROW_WORDS / 4, REQ = T::SRC_ROWS * RQ / 256;
        uint4 v[REQ];
#pragma unroll
        for (int j = 0; j < REQ; j++) {
            const int t = tid + 256 * j, r = t / RQ, c = (t % RQ) * 4;
            v[j] = make_uint4(0, 0, 0, 0);
            if (r0 + r < src_rows && c0 + c < src_cols) v[j] = ld_w16(qweight + (size_t)(r0 + r) * src_cols + c0 + c);
        }
#pragma unroll
        for (int j = 0; j < REQ; j++) {
            const int t = tid + 256 * j, r = t / RQ, c = (t % RQ) * 4;
            unsigned* p = qw + r * PITCH + c;
            p[0] = v[j].x; p[1] = v[j].y; p[2] = v[j].z; p[3] = v[j].w;
        }
    } else {
        for (int t = tid; t < T::SRC_ROWS * T::ROW_WORDS; t += 256) {
            const int r = t / T::ROW_WORDS, c = t % T::ROW_WORDS;
            if (r0 + r < src_rows && c0 + c < src_cols) qw[r * PITCH + c] = __builtin_nontemporal_load(qweight + (size_t)(r0 + r) * src_cols + c0 + c);
        }
    }

    // ---- the group tables of the tile, or its slice of g_idx
    int g0 = 0;
    if constexpr (!ACT) {
        g0 = k0 / gs;
        const int glast = (min(k0 + W4_TK, K) - 1) / gs;        // (glast - g0 < W4_MAXG)
        for (int t = tid; t < W4_MAXG * TW; t += 256) {
            const int g = g0 + t / TW, c = t % TW;
            if (g <= glast && n0 / 8 + c < nw) {
                sc4[t] = ld_w16<WLD_KEEP>(scales + (size_t)g * N + n0 + 8 * c);
                zw[t] = qzeros[(size_t)g * nw + n0 / 8 + c];
            }
        }
    } else {
        if (k0 + tid < K) {
            int g = g_idx[k0 + tid];
            if ((unsigned)g >= (unsigned)G) {                   // refused by the entry point; never an index
                flags[1] = 1u;
                g = 0;
            }
            gi[tid] = g;
        }
    }
    __syncthreads();

    if constexpr (GP) {
        const int b = quad & 7, blk = kb0 + b;
        const int gl = ACT ? 0 : (k0 + 32 * b) / gs - g0;
        for (int p = 0; p < TN / 8; p++) {
            const int nl = p * 4 + wv + 32 * (quad >> 3), n = n0 + nl;
            const bool ok = n < N && blk < nb;
            float x[8];
#pragma unroll
            for (int i = 0; i < 8; i++) x[i] = 0.0f;
            if (ok) {
                const unsigned w = qw[(4 * b + s) * PITCH + nl];
                const int zsh = 4 * (nl & 7);
                if constexpr (!ACT) {
                    const float scale = w4_widen(sc[gl * TN + nl]);
                    const int z = (int)((zw[gl * TW + (nl >> 3)] >> zsh) & 15u) + zoff;
#pragma unroll
                    for (int i = 0; i < 8; i++) x[i] = w4_value((w >> (4 * i)) & 15u, z, scale);
                } else {
                    const int* gp = gi + 32 * b + 8 * s;
#pragma unroll
                    for (int i = 0; i < 8; i++) {
                        const size_t g = (size_t)gp[i];
                        const float scale = w4_widen(scales[g * N + n]);
                        const int z = (int)((qzeros[g * nw + (n >> 3)] >> zsh) & 15u) + zoff;
                        x[i] = w4_value((w >> (4 * i)) & 15u, z, scale);
                    }
                }
            }
            w4_emit<WT>(x, ok, s, n, blk, N, nb, dst, flags);
        }
    } else {
        const int col = quad & 7, sh = 4 * ((col >> 1) + 4 * (col & 1));        // 4 P[col]
        int gl[4];
#pragma unroll
        for (int bp = 0; bp < 4; bp++) gl[bp] = (k0 + 32 * (2 * bp + (quad >> 3))) / gs - g0;
        for (int cc = 0; cc < TW / 4; cc++) {
            const int c = wv + 4 * cc, nl = 8 * c + col, n = n0 + nl;
#pragma unroll
            for (int bp = 0; bp < 4; bp++) {
                const int b = 2 * bp + (quad >> 3), blk = kb0 + b;
                const bool ok = n < N && blk < nb;
                float x[8];
#pragma unroll
                for (int i = 0; i < 8; i++) x[i] = 0.0f;
                if (ok) {
                    const float scale = w4_widen(sc[gl[bp] * TN + nl]);
                    const int z = (int)((zw[gl[bp] * TW + c] >> sh) & 15u) + zoff;
                    const unsigned* wp = qw + (32 * b + 8 * s) * PITCH + c;
#pragma unroll
                    for (int i = 0; i < 8; i++) x[i] = w4_value((wp[i * PITCH] >> sh) & 15u, z, scale);
                }
                w4_emit<WT>(x, ok, s, n, blk, N, nb, dst, flags);
            }
        }
    }
}

static unsigned* g_w4_flags = nullptr;      // two device words, zero between calls: [0] a non-finite D, [1] a g_idx entry outside [0, G)

template <int LAYOUT, bool ACT>
static int launch_w4(const void* qweight, const void* qzeros, const void* scales, const void* g_idx, int zoff, int N, int K, int gs, int G, int dst_dtype, void* dst)
{
    const int tiles_k = (K + W4_TK - 1) / W4_TK, tiles_n = (N + w4_traits<LAYOUT>::TN - 1) / w4_traits<LAYOUT>::TN;
    const auto kernel = dst_dtype == GTEN_Q8 ? k_quant_w4<LAYOUT, ACT, GTEN_Q8> : dst_dtype == GTEN_Q4 ? k_quant_w4<LAYOUT, ACT, GTEN_Q4> : k_quant_w4<LAYOUT, ACT, GTEN_F16>;
    GTR_LAUNCH(KT_PACK, kernel, dim3((unsigned)tiles_k * (unsigned)tiles_n), dim3(256), 0, (const unsigned*)qweight, (const unsigned*)qzeros,
               (const uint16_t*)scales, (const int*)g_idx, (uint8_t*)dst, N, K, gs, G, zoff, tiles_k, g_w4_flags);
    return 0;
}

// what both entry points refuse: the layout, the shape, the group size
static bool w4_shape_ok(int layout, int rows, int cols, int group_size)
{
    return (layout == GTEN_W4_GPTQ || layout == GTEN_W4_AWQ) && rows > 0 && cols > 0 && rows % 8 == 0 && cols % 32 == 0 &&
           (group_size == -1 || (group_size >= 32 && group_size % 32 == 0 && cols % group_size == 0));
}

} // namespace gtq

extern "C" size_t gten_hip_w4_src_bytes(int layout, int which, int rows, int cols, int group_size)
{
    if (!gtq::w4_shape_ok(layout, rows, cols, group_size)) return 0;
    const size_t G = group_size == -1 ? 1 : (size_t)(cols / group_size);
    switch (which) {
    case 0: return (size_t)rows * (size_t)cols / 2;
    case 1: return G * (size_t)(rows / 8) * 4;
    case 2: return G * (size_t)rows * 2;
    case 3: return layout == GTEN_W4_GPTQ ? (size_t)cols * 4 : 0;
    default: return 0;
    }
}

extern "C" int gten_hip_quantize_weight_w4(const void* qweight, const void* qzeros, const void* scales, const void* g_idx, int layout, int zero_offset,
                                           int rows, int cols, int group_size, int dst_dtype, void* dst_packed)
{
    GTR_NEED_INIT();
    GTR_REQUIRE(qweight && qzeros && scales && dst_packed && rows > 0 && cols > 0, "quantize_weight_w4: bad arguments");
    GTR_REQUIRE(layout == GTEN_W4_GPTQ || layout == GTEN_W4_AWQ, "quantize_weight_w4: layout %d is not GPTQ (0) or AWQ (1)", layout);
    GTR_REQUIRE(cols % 32 == 0 && rows % 8 == 0, "quantize_weight_w4: %d x %d: cols must be a multiple of 32 and rows a multiple of 8", rows, cols);
    GTR_REQUIRE(gtq::w4_shape_ok(layout, rows, cols, group_size), "quantize_weight_w4: group_size %d is neither -1 nor a multiple of 32 that divides cols %d",
                group_size, cols);
    GTR_REQUIRE(zero_offset == 0 || (zero_offset == 1 && layout == GTEN_W4_GPTQ), "quantize_weight_w4: zero_offset %d (0, or 1 for GPTQ)", zero_offset);
    GTR_REQUIRE(!g_idx || layout == GTEN_W4_GPTQ, "quantize_weight_w4: the AWQ layout has no g_idx");
    GTR_REQUIRE(dst_dtype == GTEN_Q8 || dst_dtype == GTEN_Q4 || dst_dtype == GTEN_F16, "quantize_weight_w4: dtype %d is not a weight dtype", dst_dtype);
    GTR_REQUIRE((((uintptr_t)qweight | (uintptr_t)qzeros | (uintptr_t)scales | (uintptr_t)g_idx | (uintptr_t)dst_packed) & 15) == 0,
                "quantize_weight_w4: sources and destination must be 16-byte aligned");
    GTR_REQUIRE((size_t)rows * cols < ((size_t)1 << 42), "quantize_weight_w4: %d x %d is too large for one launch", rows, cols);
    if (!gtq::g_w4_flags) {
        GTR_CHECK(hipMalloc((void**)&gtq::g_w4_flags, 2 * sizeof(unsigned)));
        GTR_CHECK(hipMemsetAsync(gtq::g_w4_flags, 0, 2 * sizeof(unsigned), gtr::stream()));
    }
    gtr::kv_watch_touch(dst_packed, (size_t)rows * gten_hip_row_bytes(dst_dtype, cols));
    const int gs = group_size == -1 ? cols : group_size, G = cols / gs;
    int rc;
    if (layout == GTEN_W4_AWQ) rc = gtq::launch_w4<GTEN_W4_AWQ, false>(qweight, qzeros, scales, nullptr, zero_offset, rows, cols, gs, G, dst_dtype, dst_packed);
    else if (g_idx) rc = gtq::launch_w4<GTEN_W4_GPTQ, true>(qweight, qzeros, scales, g_idx, zero_offset, rows, cols, gs, G, dst_dtype, dst_packed);
    else rc = gtq::launch_w4<GTEN_W4_GPTQ, false>(qweight, qzeros, scales, nullptr, zero_offset, rows, cols, gs, G, dst_dtype, dst_packed);
    if (rc) return rc;
    unsigned flag[2] = {0, 0};
    GTR_CHECK(hipMemcpyAsync(flag, gtq::g_w4_flags, sizeof(flag), hipMemcpyDeviceToHost, gtr::stream()));
    GTR_CHECK(hipStreamSynchronize(gtr::stream()));
    if (flag[0] | flag[1]) {
        GTR_CHECK(hipMemsetAsync(gtq::g_w4_flags, 0, sizeof(flag), gtr::stream()));
        if (flag[1]) return gtr::fail(-4, "quantize_weight_w4: g_idx holds an entry outside [0, %d), the groups of %d columns in groups of %d", G, cols, gs);
        return gtr::fail(-4, "quantize_weight_w4: a dequantised element is a NaN or an infinity: an infinite scale? (%d x %d, layout %d)", rows, cols, layout);
    }
    return 0;
}
