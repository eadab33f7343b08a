// gten_miro_math.h -- the integer arithmetic of Mirostat v2 (include/gten_hip_mirostat.h): the fixed-point log2 the
// surprise is measured with, the update of mu, and the conversion of a request to Q16.  One text for the device (gten_decode_mirostat.h),
// for the library's device-free exports (gten_hip_miro_*_host) and for a stand-alone C++ program (tests/host_miro_math.cpp): it compiles
// as device code and as plain C++ without HIP, and includes nothing but <math.h> for lrint.
//
// Surprise, tau, eta and mu are int32 in units of 2^-16 bit (Q16).  Every function here is a definition, not an approximation: the
// device, the host and the restatement in tests/miro_ref.py give the same bits.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define MIRO_FN __host__ __device__ __forceinline__
#else
#define MIRO_FN inline
#endif

#define MIRO_Q 16                        // fraction bits
#define MIRO_MU_MAX (64 << MIRO_Q)       // |mu| <= 64 bits
#define MIRO_TAU_MAX 32.f
#define MIRO_OK 0
#define MIRO_BAD_TAU 1
#define MIRO_BAD_ETA 2

// lg16(x) for x >= 1: the integer part is the position of the leading bit; the 16 fraction bits come from squaring the mantissa
// m in [2^31, 2^32) sixteen times, each square floored to 32 bits (a square that reaches 2 gives a 1 and is halved).  Monotone
// non-decreasing in x: the squaring and the floor shifts are monotone, and (bit, m) compares lexicographically.  (x == 0 is outside
// the definition; it gives 0 here so that no caller shifts by 64.)
MIRO_FN int miro_lg16(unsigned long long x)
{
    if (x == 0ull) return 0;
    const int e = 63 - __builtin_clzll(x);
    unsigned long long m = e >= 31 ? x >> (e - 31) : x << (31 - e);
    unsigned f = 0u;
    for (int i = 0; i < MIRO_Q; i++) {
        m = (m * m) >> 31;                // m < 2^32: the product fits 64 bits
        f <<= 1;
        if (m >= (1ull << 32)) { f |= 1u; m >>= 1; }
    }
    return (int)(((unsigned)e << MIRO_Q) | f);
}

// mu' = clamp(mu - ((eta_q * (s - tau_q)) >> 16), -MU_MAX, MU_MAX): the product in 64 bits, the shift arithmetic (a floor, not a
// truncation, for a negative product)
MIRO_FN int miro_update(int mu, int s, int tau_q, int eta_q)
{
    const long long step = ((long long)eta_q * (long long)(s - tau_q)) >> MIRO_Q;
    long long v = (long long)mu - (long long)(int)step;
    if (v > (long long)MIRO_MU_MAX) v = (long long)MIRO_MU_MAX;
    if (v < -(long long)MIRO_MU_MAX) v = -(long long)MIRO_MU_MAX;
    return (int)v;
}

// the smallest mass T in [1, 2^bits] with lg16(T) >= L, or 2^bits + 1 where there is none: lg16 is monotone, so {q >= 1 :
// lg16(q) >= L} = {q >= T} and a row compares masses instead of logarithms
MIRO_FN unsigned long long miro_threshold(int L, int bits)
{
    unsigned long long lo = 1ull, hi = (1ull << bits) + 1ull;
    while (lo < hi) {
        const unsigned long long mid = lo + ((hi - lo) >> 1);
        if (miro_lg16(mid) >= L) hi = mid; else lo = mid + 1ull;
    }
    return lo;
}

// a request to Q16, formed once on the host when the request is set: 0 < tau <= 32, 0 < eta <= 1, both finite
inline int miro_q16(float tau, float eta, int* tau_q, int* eta_q)
{
    if (!(tau > 0.f && tau <= MIRO_TAU_MAX)) return MIRO_BAD_TAU;        // (a NaN fails every comparison)
    if (!(eta > 0.f && eta <= 1.f)) return MIRO_BAD_ETA;
    *tau_q = (int)lrint((double)tau * 65536.0);
    *eta_q = (int)lrint((double)eta * 65536.0);
    return MIRO_OK;
}
