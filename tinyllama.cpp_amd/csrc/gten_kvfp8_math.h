// gten_kvfp8_math.h -- the rounding R of the FP8 (OCP E4M3) head-major K / V shadows of the f16 wide decoders (DESIGN.md §3.25,
// include/gten_hip_kvfp8.h).  Device-free and integer-only: the kernels (gten_decode_attn_hm_kernels.h, gten_decode_kvfp8.h) and a
// stand-alone host program (tests/host_kvfp8_math.cpp) share this text; tests/kv_fp8_ref.py restates the contract on its own.
//
// An E4M3 code is {sign, 4 exponent bits E, 3 mantissa bits m}: E >= 1 is (1 + m / 8) 2^(E - 7), E = 0 is the subnormal m 2^-9, the
// largest finite value is 448 (0x7e), and 0x7f / 0xff are NaN -- 253 distinct finite values, every one of them an f16 value.
//     R8   f16 bits -> code: the nearest of the 253 values, ties to the even code; |x| beyond 448 (infinities too) -> +-448; NaN -> +0;
//          -0 and everything that rounds to zero keep their sign.  0x7f and 0xff are never produced.
//     E8   code -> f16 bits, exact.
//     R  = E8 o R8 per element: deterministic (it reads 2 bytes), and idempotent because R8(E8(c)) = c for every code R8 produces
//          (an E4M3 value is its own nearest value) -- a shadow built by appends and one built by an import hold the same bytes, and
//          an f16-shadow decoder on rows rounded by R computes what an FP8 decoder computes on the unrounded rows.
// How R8 rounds: with a = |x|'s 15 bits, a value of at least 2^-6 (a >= 9 << 10) has E = e16 - 8 and loses the low 7 of its 10
// mantissa bits, so (a - (8 << 10)) >> 7 IS the truncated code and the lost bits decide the rounding (a carry runs into E, as it
// must; past 0x7e it is the clamp).  Below 2^-6 the grid is m 2^-9: the significand (1024 | m16, or m16 alone for an f16
// subnormal) shifted right by 16 - max(e16, 1), in 8 .. 15, is m, and what is shifted out decides; m = 8 is the code of 2^-6.
#ifndef GTEN_KVFP8_MATH_H
#define GTEN_KVFP8_MATH_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KVFP8_FN __host__ __device__ __forceinline__
#else
#define KVFP8_FN static inline
#endif

#define KVFP8_MAX_CODE 0x7eu      // 448

KVFP8_FN uint8_t kvfp8_r8(uint16_t h)
{
    const uint32_t s = ((uint32_t)h >> 8) & 0x80u, a = (uint32_t)h & 0x7fffu;
    if (a > 0x7c00u) return (uint8_t)0;                            // NaN
    uint32_t code, rem, half;
    if (a >= (9u << 10)) {
        const uint32_t x = a - (8u << 10);
        code = x >> 7;
        rem = x & 0x7fu;
        half = 0x40u;
    } else {
        const uint32_t e = a >> 10, sig = e ? (1024u | (a & 1023u)) : a, sh = 16u - (e ? e : 1u);
        code = sig >> sh;
        rem = sig & ((1u << sh) - 1u);
        half = 1u << (sh - 1u);
    }
    if (rem > half || (rem == half && (code & 1u))) code++;
    if (code > KVFP8_MAX_CODE) code = KVFP8_MAX_CODE;              // (the infinities arrive here too)
    return (uint8_t)(s | code);
}

KVFP8_FN uint16_t kvfp8_e8(uint8_t c)
{
    const uint32_t s = ((uint32_t)c & 0x80u) << 8, E = ((uint32_t)c >> 3) & 15u, m = (uint32_t)c & 7u;
    if (E) return (uint16_t)(s | ((E + 8u) << 10) | (m << 7));
    if (m == 0) return (uint16_t)s;
    // m 2^-9 as a normal half: the leading one of m at bit b is 2^(b - 9), e16 = b + 6
    const uint32_t b = m >= 4u ? 2u : m >= 2u ? 1u : 0u;
    return (uint16_t)(s | ((b + 6u) << 10) | (((m << (10u - b)) & 1023u)));
}

KVFP8_FN uint16_t kvfp8_round(uint16_t h) { return kvfp8_e8(kvfp8_r8(h)); }

// ---- the FP8 shadow chunk of 256 positions of one kv head (gten_decode_attn_hm.h describes it): byte offset of the code of element
// e in [0, 64) of position p in [0, 256), K and V, in [0, HMF8_CHUNK_BYTES)
#define HMF8_CHUNK_BYTES 16384
KVFP8_FN unsigned hmf8_k_off(unsigned p, unsigned e)
{
    return (p >> 4) * 1024u + (((((e & 31u) >> 3) * 16u) + (p & 15u)) * 16u) + (e >> 5) * 8u + (e & 7u);
}
KVFP8_FN unsigned hmf8_v_off(unsigned p, unsigned e)
{
    return (p >> 5) * 2048u + (e >> 5) * 1024u + (((((p & 15u) >> 2) * 16u) + (e & 15u)) * 16u) + ((e >> 4) & 1u) * 8u + 4u * ((p >> 4) & 1u) + (p & 3u);
}
#endif
