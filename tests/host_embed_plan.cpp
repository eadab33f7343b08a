// host_embed_plan.cpp -- host/embed_plan.h alone, under ASan + UBSan (tests/test_embed_cpu.py): the plan over length lists with
// exactly sized outputs, its invariants checked one by one, and the cases the rule turns on.
#include "../tinyllama.cpp_amd/host/embed_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace gten;

#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

// the invariants of a plan: groups numbered by first text, a text alone exactly where the rule says, grouped texts within the caps,
// and no group opened while the open one still had room
static void check(const std::vector<int>& len, bool seg_ok)
{
    const int n = (int)len.size();
    std::vector<int> group_of((size_t)n, -7), alone((size_t)n, -7);       // exactly n entries each: an overrun is ASan's to find
    const int G = embed_plan(len.data(), n, seg_ok, group_of.data(), alone.data());
    CHECK(G >= 1 && G <= n);
    CHECK(embed_plan(len.data(), n, seg_ok, nullptr, nullptr) == G);
    std::vector<int> texts((size_t)G, 0), rows((size_t)G, 0);
    int seen = 0, open = -1;
    for (int k = 0; k < n; k++) {
        const int g = group_of[(size_t)k];
        CHECK(g >= 0 && g < G && g <= seen);
        const bool grouped = embed_grouped(len[(size_t)k], seg_ok);
        CHECK(grouped == (seg_ok && len[(size_t)k] >= 16 && len[(size_t)k] <= 2048));
        CHECK(alone[(size_t)g] == (grouped ? 0 : 1));
        if (g == seen) {                                                  // a new group
            seen++;
            if (grouped) {
                if (open >= 0) CHECK(texts[(size_t)open] == kEmbedGroupTexts || rows[(size_t)open] + len[(size_t)k] > kEmbedGroupRows);
                open = g;
            }
        } else {
            CHECK(grouped && g == open);                                  // only the open group grows
        }
        texts[(size_t)g]++;
        rows[(size_t)g] += len[(size_t)k];
    }
    CHECK(seen == G);
    for (int g = 0; g < G; g++) {
        CHECK(alone[(size_t)g] == 0 || alone[(size_t)g] == 1);
        if (alone[(size_t)g]) CHECK(texts[(size_t)g] == 1);
        else CHECK(texts[(size_t)g] >= 1 && texts[(size_t)g] <= kEmbedGroupTexts && rows[(size_t)g] <= kEmbedGroupRows);
    }
}

int main()
{
    long plans = 0;
    const int lens[] = {1, 15, 16, 17, 64, 127, 128, 129, 2047, 2048, 2049, 5000};
    for (int a : lens)
        for (int b : lens)
            for (int c : lens)
                for (int seg = 0; seg < 2; seg++) {
                    check({a}, seg != 0);
                    check({a, b}, seg != 0);
                    check({a, b, c, a}, seg != 0);
                    plans += 3;
                }
    // a 33rd text opens a second group; 32 texts of 128 rows fill one exactly; one more row does not fit
    for (int n : {1, 31, 32, 33, 64, 65, 100}) {
        check(std::vector<int>((size_t)n, 16), true);
        check(std::vector<int>((size_t)n, 128), true);
        check(std::vector<int>((size_t)n, 129), true);
        check(std::vector<int>((size_t)n, 2048), true);
        check(std::vector<int>((size_t)n, 9), true);
        plans += 5;
    }
    {
        std::vector<int> g(33), al(33);
        std::vector<int> len(33, 16);
        CHECK(embed_plan(len.data(), 33, true, g.data(), al.data()) == 2 && g[31] == 0 && g[32] == 1);
        len.assign(32, 128);
        CHECK(embed_plan(len.data(), 32, true, g.data(), al.data()) == 1);
        len[31] = 129;
        CHECK(embed_plan(len.data(), 32, true, g.data(), al.data()) == 2 && g[30] == 0 && g[31] == 1);
        // a text that goes alone does not close the open group
        const int mixed[] = {20, 5, 30};
        CHECK(embed_plan(mixed, 3, true, g.data(), al.data()) == 2 && g[0] == 0 && g[1] == 1 && g[2] == 0 && al[0] == 0 && al[1] == 1);
        CHECK(embed_plan(mixed, 3, false, g.data(), al.data()) == 3 && al[0] == 1 && al[1] == 1 && al[2] == 1);
        const int bad[] = {20, 0, 30};
        CHECK(embed_plan(bad, 3, true, g.data(), al.data()) == -1);
        CHECK(embed_plan(mixed, 0, true, g.data(), al.data()) == -1);
        CHECK(embed_plan(nullptr, 3, true, g.data(), al.data()) == -1);
    }
    // a long pseudo-random list
    {
        std::vector<int> len;
        unsigned s = 12345u;
        for (int i = 0; i < 3000; i++) {
            s = s * 1664525u + 1013904223u;
            len.push_back(1 + (int)((s >> 8) % ((s >> 30) ? 300u : 2100u)));
        }
        check(len, true);
        check(len, false);
        plans += 2;
    }
    std::printf("host_embed_plan ok: %ld plans\n", plans);
    return 0;
}
