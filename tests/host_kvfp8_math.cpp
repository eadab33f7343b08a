// host_kvfp8_math.cpp -- csrc/gten_kvfp8_math.h alone, under ASan + UBSan (tests/test_kv_fp8_cpu.py): over all 65 536 f16 patterns R8
// against a brute-force nearest-value search in double, R idempotent, E8 exact; the chunk's offset functions bijections onto [0, 16384).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../tinyllama.cpp_amd/csrc/gten_kvfp8_math.h"

static long checks = 0;
#define CHECK(c) do { checks++; if (!(c)) { std::printf("host_kvfp8_math: %s failed at line %d (h = 0x%04x)\n", #c, __LINE__, h); std::exit(1); } } while (0)

static double half_value(unsigned h)              // a finite f16 pattern, exactly
{
    const int e = (h >> 10) & 31, m = h & 1023;
    return ((h & 0x8000u) ? -1.0 : 1.0) * (e ? std::ldexp(1024.0 + m, e - 25) : std::ldexp((double)m, -24));
}
static double code_value(unsigned c)              // an E4M3 code other than NaN, by the format's definition
{
    const int E = (c >> 3) & 15, m = c & 7;
    return ((c & 0x80u) ? -1.0 : 1.0) * (E ? std::ldexp(8.0 + m, E - 10) : std::ldexp((double)m, -9));
}

int main()
{
    unsigned h = 0;
    // E8 is exact on every code, and R8 returns every finite code from its own value
    for (unsigned c = 0; c < 256; c++) {
        h = kvfp8_e8((uint8_t)c);
        CHECK(((h >> 10) & 31u) != 31u && half_value(h) == code_value(c));
        if ((c & 0x7fu) != 0x7fu) CHECK(kvfp8_r8((uint16_t)h) == c);
    }
    for (h = 0; h < 65536u; h++) {
        const unsigned c = kvfp8_r8((uint16_t)h), e = (h >> 10) & 31u, m = h & 1023u;
        CHECK((c & 0x7fu) != 0x7fu);
        if (e == 31u && m) { CHECK(c == 0); continue; }            // NaN -> +0
        CHECK((c >> 7) == (h >> 15));                              // the sign stays, also on what rounds to zero
        // the nearest magnitude among codes 0 .. 0x7e; a tie takes the even code (neighbouring codes differ in parity)
        const double x = e == 31u ? INFINITY : std::fabs(half_value(h));
        unsigned best = 0;
        for (unsigned k = 1; k <= KVFP8_MAX_CODE; k++) {
            const double dk = std::fabs(code_value(k) - x), db = std::fabs(code_value(best) - x);
            if (dk < db || (dk == db && !(k & 1u))) best = k;
        }
        if (e == 31u) best = KVFP8_MAX_CODE;                       // (inf - v is inf for every v: the contract says 448)
        CHECK((c & 0x7fu) == best);
        const unsigned r = kvfp8_round((uint16_t)h);
        CHECK(kvfp8_round((uint16_t)r) == r && kvfp8_r8((uint16_t)r) == c);
    }
    h = 0;
    for (int kv = 0; kv < 2; kv++) {
        std::vector<int> seen(HMF8_CHUNK_BYTES, 0);
        for (unsigned p = 0; p < 256; p++)
            for (unsigned e = 0; e < 64; e++) {
                const unsigned o = kv ? hmf8_v_off(p, e) : hmf8_k_off(p, e);
                CHECK(o < HMF8_CHUNK_BYTES);
                seen[o]++;
            }
        for (int n : seen) CHECK(n == 1);
    }
    std::printf("host_kvfp8_math ok (%ld checks)\n", checks);
    return 0;
}
