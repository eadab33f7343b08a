// gten_kvq4_math.h -- "Q4 of a Q8 block": the rounding R of the 4-bit head-major K / V shadows (DESIGN.md §3.24,
// include/gten_hip_kvq4.h).  Device-free: the kernels (gten_decode_attn_hm_kernels.h, gten_decode_kvq4.h), a stand-alone host
// program (tests/host_kvq4_math.cpp) and, operation for operation, the NumPy restatement (tests/kv_q4_ref.py) share this text.
//
// R takes a Q8 block {f16 d, int8 q[32]} to {f16 d4, q4[32]} with q4 in [-7, 7] -- again a Q8 block, of 15 levels:
//     m    = max |q[i]|                                   (an integer, 0 .. 128)
//     x    = f32(m) * |f32(d)| / 7                        the product is exact (8 x 11 bits); ONE f32 division, rounded to nearest
//     d4   = 0                   if d is not finite, or x < 2^-14 (m = 0, d = 0, and blocks whose delta would be a subnormal half)
//          = min(f16(x), 65504)  otherwise                f32 -> f16 rounded to nearest even; an overflow stays the largest half
//     q4_i = clamp(rne(f32(q_i) * f32(d) / f32(d4)), -7, 7)   exact product, ONE f32 division, round half to even; all 0 if d4 = 0
// Every step is an IEEE operation on f32 values that are normal or zero (m |d| >= 2^-24, d4 >= 2^-14), so flush-to-zero modes,
// f64 evaluation with a rounding to f32 at the two divisions, and the device's v_div sequences all give the same bits.
//
// Two properties (the tests hold the code to both; tests/host_kvq4_math.cpp sweeps every d):
//   1. R is DETERMINISTIC PER BLOCK: it reads nothing but the block's 34 bytes.  An import of a row and an append of the same row
//      therefore leave the same shadow bytes, whoever runs first and whatever lies beside the block.
//   2. R is IDEMPOTENT, R(R(b)) == R(b) byte for byte.  Proof.  d4 = 0: R(b) is the zero block, m = 0 on the second pass, x = 0,
//      zero block again.  Otherwise D = f32(d4) is a NORMAL half, 2^-14 <= D <= 65504, and the largest |q4| is exactly 7:
//        - D = f16(x) not clamped: D = x (1 + e) with |e| <= 2^-11, the largest quotient is m |d| / D = 7 x' / D where x' is x before
//          its f32 rounding, so it lies within 7 (1 +- 2^-10) and rounds to 7;
//        - D clamped to 65504 < x: the largest quotient exceeds 7 and is clamped to 7.
//      Second pass: m' = 7 and x = f32(7) * D / 7.  7 D has at most 14 significant bits, so the product is exact and the division
//      returns D exactly; D >= 2^-14 is not flushed, f16(D) = D, no clamp: d4' = d4.  Then q4'_i = rne(q4_i * D / D) = q4_i: the
//      product is exact (4 x 11 bits), the quotient is the integer itself, and it is within [-7, 7].                          qed
// (Without the 2^-14 floor idempotence fails: x = 1.5 * 2^-24 rounds to the half 2^-23, the largest quotient is 5.25 -> 5, and the
//  second pass sees x = 10/7 * 2^-24 -> 2^-24, another delta.  Such a block's values are below 4.3e-4 in magnitude; R calls it zero.)
#ifndef GTEN_KVQ4_MATH_H
#define GTEN_KVQ4_MATH_H
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KVQ4_FN __host__ __device__ __forceinline__
#else
#define KVQ4_FN static inline
#endif

#define KVQ4_LEVEL 7              // |q4| <= 7
#define KVQ4_BIAS 8               // a stored nibble is q4 + 8, in [1, 15]

KVQ4_FN float kvq4_bits_f32(uint32_t u)
{
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
KVQ4_FN uint32_t kvq4_f32_bits(float f)
{
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    return u;
}
// f16 bits -> f32, exact (integer operations: the same on every side)
KVQ4_FN float kvq4_h2f(uint16_t h)
{
    const uint32_t s = ((uint32_t)h & 0x8000u) << 16, e = ((uint32_t)h >> 10) & 31u, m = (uint32_t)h & 1023u;
    if (e == 0) {
        const float f = (float)m * 5.9604644775390625e-8f;       // m * 2^-24, exact
        return kvq4_bits_f32(kvq4_f32_bits(f) | s);
    }
    if (e == 31) return kvq4_bits_f32(s | 0x7f800000u | (m << 13));
    return kvq4_bits_f32(s | ((e + 112u) << 23) | (m << 13));
}
// a finite f32 x >= 2^-14 -> f16 bits, rounded to nearest even, an overflow clamped to 65504 (0x7bff)
KVQ4_FN uint16_t kvq4_f2h_normal(float x)
{
    const uint32_t u = kvq4_f32_bits(x);
    if (u >= 0x47800000u) return (uint16_t)0x7bffu;               // >= 65536: past every half
    uint32_t h = (((u >> 23) - 112u) << 10) | ((u >> 13) & 1023u);
    const uint32_t rem = u & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) h++;       // (a carry runs into the exponent, as it must)
    return (uint16_t)(h > 0x7bffu ? 0x7bffu : h);
}
// the delta of R(b) from the block's largest |q| and its delta
KVQ4_FN uint16_t kvq4_delta(int maxabs, uint16_t d_bits)
{
    if (((d_bits >> 10) & 31u) == 31u) return (uint16_t)0;        // d is not finite
    const float x = (float)maxabs * fabsf(kvq4_h2f(d_bits)) / 7.0f;
    if (!(x >= 6.103515625e-5f)) return (uint16_t)0;              // below 2^-14 (and m = 0, d = 0)
    return kvq4_f2h_normal(x);
}
// one element of R(b): q under the block's delta d_bits, requantized to the delta d4_bits = kvq4_delta(...)
KVQ4_FN int kvq4_quant(int q, uint16_t d_bits, uint16_t d4_bits)
{
    if (d4_bits == 0) return 0;
    const float r = rintf((float)q * kvq4_h2f(d_bits) / kvq4_h2f(d4_bits));
    return r > 7.0f ? 7 : r < -7.0f ? -7 : (int)r;
}
// a whole block in place: blk = {f16 d, int8 q[32]} as 34 bytes at any even address
KVQ4_FN void kvq4_round_block(uint8_t* blk)
{
    const uint16_t d = (uint16_t)(blk[0] | (blk[1] << 8));
    int m = 0;
    for (int i = 0; i < 32; i++) {
        const int q = (int8_t)blk[2 + i];
        m = (q < 0 ? -q : q) > m ? (q < 0 ? -q : q) : m;
    }
    const uint16_t d4 = kvq4_delta(m, d);
    for (int i = 0; i < 32; i++) blk[2 + i] = (uint8_t)(int8_t)kvq4_quant((int8_t)blk[2 + i], d, d4);
    blk[0] = (uint8_t)(d4 & 0xffu);
    blk[1] = (uint8_t)(d4 >> 8);
}

// ---- the 4-bit shadow chunk of 256 positions of one kv head (gten_decode_attn_hm.h describes it): position p in [0, 256), element e in
// [0, 64), quant block / half in {0, 1}.  hmq4_*_q_off: NIBBLE index in [0, 16384) -- byte = index >> 1, high nibble = index & 1;
// hmq4_*_d_off: byte offset of the f16 delta in [8192, 9216), the Q8 chunk's delta layout behind the nibbles.
#define HMQ4_CHUNK_BYTES 9216
#define HMQ4_Q_BYTES 8192
KVQ4_FN unsigned hmq4_k_q_off(unsigned p, unsigned e)
{
    return ((p >> 5) * 1024u + (((e >> 4) * 16u + (p & 15u)) * 16u) + (e & 15u)) * 2u + ((p >> 4) & 1u);
}
KVQ4_FN unsigned hmq4_k_d_off(unsigned p, unsigned blk) { return HMQ4_Q_BYTES + blk * 512u + ((p & 15u) >> 2) * 128u + (p >> 4) * 8u + (p & 3u) * 2u; }
KVQ4_FN unsigned hmq4_v_q_off(unsigned p, unsigned e)
{
    const unsigned s = p >> 5, r = p & 15u, j = 4u * ((p >> 4) & 1u) + (r & 3u), bit = 4u * (j >> 1) + 16u * (j & 1u);
    return (s * 1024u + (((r >> 2) * 16u + (e & 15u)) * 16u) + (e >> 4) * 4u) * 2u + (bit >> 2);
}
KVQ4_FN unsigned hmq4_v_d_off(unsigned p, unsigned half)
{
    const unsigned s = p >> 5, tp = (p >> 4) & 1u, r = p & 15u;
    return HMQ4_Q_BYTES + ((r >> 2) * 2u + ((r >> 1) & 1u)) * 128u + s * 16u + (tp * 4u + (r & 1u) * 2u + half) * 2u;
}
#endif
