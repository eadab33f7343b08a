// host_miro_math.cpp -- csrc/gten_miro_math.h alone, under ASan + UBSan (tests/test_mirostat_cpu.py): lg16 at its edges and on a sweep,
// its monotony, the threshold against its definition, the update's clamps and floor, the Q16 conversion's refusals.  A stand-alone
// program: the header is device-free, so what the device and the library run is what runs here.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>

#include "../tinyllama.cpp_amd/csrc/gten_miro_math.h"

static long checks = 0;
#define CHECK(c) do { checks++; if (!(c)) { std::printf("host_miro_math: %s failed at line %d\n", #c, __LINE__); std::exit(1); } } while (0)

int main()
{
    // lg16: known values, every power of two and its neighbours
    CHECK(miro_lg16(1ull) == 0 && miro_lg16(2ull) == (1 << 16) && miro_lg16(1ull << 36) == (36 << 16) && miro_lg16(0ull) == 0);
    for (int k = 1; k < 64; k++) {
        const unsigned long long p = 1ull << k;
        CHECK(miro_lg16(p) == (k << 16));
        CHECK(miro_lg16(p - 1ull) <= miro_lg16(p) && miro_lg16(p) <= miro_lg16(p + 1ull));
        CHECK(miro_lg16(p - 1ull) >= ((k - 1) << 16) && miro_lg16(p + 1ull) < ((k + 1) << 16));
    }
    CHECK(miro_lg16(~0ull) < (64 << 16) && miro_lg16(~0ull) >= (63 << 16));
    // monotone on a dense sweep of small values and on a geometric sweep up to 2^63
    int last = 0;
    for (unsigned long long x = 1ull; x < 300000ull; x++) { const int l = miro_lg16(x); CHECK(l >= last); last = l; }
    last = 0;
    for (unsigned long long x = 1ull; x < (1ull << 63); x += (x >> 7) + 1ull) { const int l = miro_lg16(x); CHECK(l >= last); last = l; }
    // the threshold: the smallest mass whose lg16 reaches L -- checked against the definition on both of its sides
    for (int L = -(70 << 16); L <= (40 << 16); L += 12345) {
        const unsigned long long T = miro_threshold(L, 36);
        CHECK(T >= 1ull && T <= (1ull << 36) + 1ull);
        if (T <= (1ull << 36)) CHECK(miro_lg16(T) >= L);
        if (T > 1ull) CHECK(miro_lg16(T - 1ull) < L);
    }
    CHECK(miro_threshold(0, 36) == 1ull && miro_threshold(-5, 36) == 1ull && miro_threshold(1, 36) == 2ull);
    CHECK(miro_threshold(36 << 16, 36) == (1ull << 36) && miro_threshold((36 << 16) + 1, 36) == (1ull << 36) + 1ull);
    CHECK(miro_threshold(std::numeric_limits<int>::max(), 36) == (1ull << 36) + 1ull && miro_threshold(std::numeric_limits<int>::min(), 36) == 1ull);
    // the update: the floor of a negative product, both clamps, the extremes of every argument
    CHECK(miro_update(0, 1, 2, 1) == 1 && miro_update(0, 2, 1, 1) == 0);
    CHECK(miro_update(10 << 16, 5 << 16, 5 << 16, 6554) == (10 << 16));
    CHECK(miro_update(10 << 16, 0, 5 << 16, 6554) == (10 << 16) + 32770);
    CHECK(miro_update(MIRO_MU_MAX, 0, 32 << 16, 65536) == MIRO_MU_MAX && miro_update(-MIRO_MU_MAX, 63 << 16, 1, 65536) == -MIRO_MU_MAX);
    CHECK(miro_update(MIRO_MU_MAX, 64 << 16, 1, 65536) == MIRO_MU_MAX - (64 << 16) + 1);
    for (int mu = -MIRO_MU_MAX; mu <= MIRO_MU_MAX; mu += 65537)
        for (int s = 0; s <= (64 << 16); s += 99991)
            for (int eta_q = 0; eta_q <= 65536; eta_q += 8192) {
                const int v = miro_update(mu, s, 3 << 16, eta_q);
                CHECK(v >= -MIRO_MU_MAX && v <= MIRO_MU_MAX);
                if (eta_q == 0) CHECK(v == mu);
                if (s > (3 << 16)) CHECK(v <= mu); else CHECK(v >= mu);
            }
    // Q16
    int t = -1, e = -1;
    CHECK(miro_q16(5.f, 0.1f, &t, &e) == MIRO_OK && t == (5 << 16) && e == 6554);
    CHECK(miro_q16(32.f, 1.f, &t, &e) == MIRO_OK && t == (32 << 16) && e == 65536);
    CHECK(miro_q16(1e-9f, 1e-9f, &t, &e) == MIRO_OK && t == 0 && e == 0);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    t = e = -7;
    for (float bad : {0.f, -1.f, 32.001f, nan, inf, -inf}) CHECK(miro_q16(bad, 0.1f, &t, &e) == MIRO_BAD_TAU);
    for (float bad : {0.f, -0.1f, 1.0001f, nan, inf, -inf}) CHECK(miro_q16(5.f, bad, &t, &e) == MIRO_BAD_ETA);
    CHECK(t == -7 && e == -7);                         // a refusal writes nothing
    std::printf("host_miro_math ok (%ld checks)\n", checks);
    return 0;
}
