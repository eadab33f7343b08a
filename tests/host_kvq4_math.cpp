// host_kvq4_math.cpp -- csrc/gten_kvq4_math.h alone, under ASan + UBSan (tests/test_kv_q4_cpu.py).  Without arguments: R's idempotence
// over EVERY f16 delta and a sweep of quant patterns, its range, and the 4-bit chunk's offset functions as bijections.  With two file
// names: R on every 34-byte block of the first file, written to the second (the test compares that with tests/kv_q4_ref.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../tinyllama.cpp_amd/csrc/gten_kvq4_math.h"

static long checks = 0;
#define CHECK(c) do { checks++; if (!(c)) { std::printf("host_kvq4_math: %s failed at line %d\n", #c, __LINE__); std::exit(1); } } while (0)

static void fill(uint8_t* blk, uint16_t d, int pattern, unsigned& rng)
{
    blk[0] = (uint8_t)(d & 0xff);
    blk[1] = (uint8_t)(d >> 8);
    for (int i = 0; i < 32; i++) {
        rng = rng * 1664525u + 1013904223u;
        int q = (int)((rng >> 16) & 255u) - 128;
        // all zero | a single non-zero | 127 | -128 | small, with ties at the maximum | already 15 levels | random
        const int pat[6] = {0, i == 11 ? -1 : 0, i == 3 ? 127 : q / 2, i == 30 ? -128 : q / 4, q / 19, (i & 1) ? 7 : -7};
        blk[2 + i] = (uint8_t)(int8_t)(pattern < 6 ? pat[pattern] : q);
    }
}

int main(int argc, char** argv)
{
    if (argc == 3) {
        std::FILE* f = std::fopen(argv[1], "rb");
        if (!f) return 2;
        std::vector<uint8_t> buf;
        uint8_t tmp[34];
        while (std::fread(tmp, 1, 34, f) == 34) { kvq4_round_block(tmp); buf.insert(buf.end(), tmp, tmp + 34); }
        std::fclose(f);
        f = std::fopen(argv[2], "wb");
        if (!f || std::fwrite(buf.data(), 1, buf.size(), f) != buf.size()) return 2;
        std::fclose(f);
        return 0;
    }
    // the half conversions on every half: exact round trip of every normal half, the clamp at the top
    for (unsigned h = 0x0400; h <= 0x7bff; h++) CHECK(kvq4_f2h_normal(kvq4_h2f((uint16_t)h)) == h);
    CHECK(kvq4_f2h_normal(65519.0f) == 0x7bff && kvq4_f2h_normal(65520.0f) == 0x7bff && kvq4_f2h_normal(1e30f) == 0x7bff);
    CHECK(kvq4_h2f(0x0001) == 5.9604644775390625e-8f && kvq4_h2f(0x3c00) == 1.0f && kvq4_h2f(0xc000) == -2.0f);
    // idempotence and range over all 65536 deltas x 7 patterns (x 3 draws of the random ones)
    unsigned rng = 12345u;
    uint8_t a[34], b[34];
    for (unsigned d = 0; d < 65536u; d++)
        for (int pattern = 0; pattern < 9; pattern++) {
            fill(a, (uint16_t)d, pattern, rng);
            kvq4_round_block(a);
            std::memcpy(b, a, 34);
            kvq4_round_block(b);
            CHECK(std::memcmp(a, b, 34) == 0);
            const unsigned d4 = a[0] | (a[1] << 8);
            CHECK(d4 == 0 || (d4 >= 0x0400 && d4 <= 0x7bff));       // zero, or a positive normal half
            int m = 0;
            for (int i = 0; i < 32; i++) { const int q = (int8_t)a[2 + i]; CHECK(q >= -7 && q <= 7); m = (q < 0 ? -q : q) > m ? (q < 0 ? -q : q) : m; }
            CHECK(m == (d4 ? 7 : 0));                              // the largest element sits on the outermost level
        }
    // the chunk layout: the quant offsets are a bijection onto the 16384 nibbles, the delta offsets onto the half-words behind them
    for (int kv = 0; kv < 2; kv++) {
        std::vector<int> nib(2 * HMQ4_Q_BYTES, 0), del(HMQ4_CHUNK_BYTES, 0);
        for (unsigned p = 0; p < 256; p++) {
            for (unsigned e = 0; e < 64; e++) {
                const unsigned i = kv ? hmq4_v_q_off(p, e) : hmq4_k_q_off(p, e);
                CHECK(i < 2u * HMQ4_Q_BYTES);
                nib[i]++;
            }
            for (unsigned h = 0; h < 2; h++) {
                const unsigned o = kv ? hmq4_v_d_off(p, h) : hmq4_k_d_off(p, h);
                CHECK(o >= HMQ4_Q_BYTES && o + 2 <= HMQ4_CHUNK_BYTES && o % 2 == 0);
                del[o]++;
            }
        }
        for (int c : nib) CHECK(c == 1);
        for (unsigned o = HMQ4_Q_BYTES; o < HMQ4_CHUNK_BYTES; o += 2) CHECK(del[o] == 1);
    }
    std::printf("host_kvq4_math ok (%ld checks)\n", checks);
    return 0;
}
