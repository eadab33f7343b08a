// host_resident_plan.cpp -- cases for host/resident_plan.h (which W.x launches of a decode step keep their weights in the memory-side
// cache) on TinyLlama's launch list in q4, q8 and f16 and on a two-layer toy list; built plain and with -fsanitize=address,undefined
// by tests/test_resident_plan_cpu.py.  Includes that header alone: no device, no model.
#include "../tinyllama.cpp_amd/host/resident_plan.h"

#include <cstdio>
#include <cstdlib>

using namespace gten;

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            std::fprintf(stderr, "host_resident_plan: line %d: %s\n", __LINE__, #cond); \
            std::exit(1);                                                               \
        }                                                                               \
    } while (0)

static long long total_bytes(const std::vector<ResidentLaunch>& step)
{
    long long t = 0;
    for (const ResidentLaunch& l : step) t += l.bytes;
    return t;
}

static int count_family(const std::vector<ResidentLaunch>& step, const ResidentPlan& p, int family)
{
    int n = 0;
    for (size_t i = 0; i < step.size(); i++) n += (p.resident[i] && step[i].family == family) ? 1 : 0;
    return n;
}

// what every plan must satisfy, whatever the list and the budget
static void consistent(const std::vector<ResidentLaunch>& step, const ResidentPlan& p, long long budget)
{
    CHECK(p.resident.size() == step.size());
    long long sum = 0, largest_in = -1, smallest_out = -1;
    int n = 0;
    for (size_t i = 0; i < step.size(); i++) {
        CHECK(p.resident[i] == 0 || p.resident[i] == 1);
        if (p.resident[i]) { n++; sum += step[i].bytes; largest_in = std::max(largest_in, step[i].bytes); }
        else if (smallest_out < 0 || step[i].bytes < smallest_out) smallest_out = step[i].bytes;
    }
    CHECK(n == p.launches && sum == p.bytes);
    CHECK(p.bytes <= std::max(budget, 0ll));                              // never above the budget
    if (smallest_out >= 0 && largest_in >= 0) CHECK(largest_in <= smallest_out);   // the smallest launches, nothing squeezed in behind
    if (smallest_out >= 0) CHECK(p.bytes + smallest_out > budget);        // ... and the next one really did not fit
    // with equal sizes, earlier launches win: a resident launch has no earlier non-resident launch of its size
    for (size_t i = 0; i < step.size(); i++)
        for (size_t j = i + 1; j < step.size(); j++)
            if (step[i].bytes == step[j].bytes) CHECK(p.resident[i] >= p.resident[j]);
}

static void sweep(const std::vector<ResidentLaunch>& step)
{
    const long long all = total_bytes(step);
    long long smallest = step[0].bytes;
    for (const ResidentLaunch& l : step) smallest = std::min(smallest, l.bytes);
    // budget 0, a budget below the smallest launch, a negative one: nobody; everything: everybody
    for (long long b : {0ll, 1ll, smallest - 1, -5ll}) {
        const ResidentPlan p = resident_plan(step, b);
        consistent(step, p, b);
        CHECK(p.launches == 0 && p.bytes == 0);
    }
    for (long long b : {all, all + 1, 4 * all}) {
        const ResidentPlan p = resident_plan(step, b);
        consistent(step, p, b);
        CHECK(p.launches == (int)step.size() && p.bytes == all);
    }
    CHECK(resident_plan(step, all - 1).launches == (int)step.size() - 1);
    CHECK(resident_plan(step, smallest).launches == 1);
    // monotone: raising the budget never drops a launch (steps that straddle every launch size)
    ResidentPlan prev = resident_plan(step, 0);
    const long long inc = std::max(1ll, smallest / 3);
    for (long long b = 0; b <= all + inc; b += inc) {
        const ResidentPlan p = resident_plan(step, b);
        consistent(step, p, b);
        CHECK(p.launches >= prev.launches && p.bytes >= prev.bytes);
        for (size_t i = 0; i < step.size(); i++) CHECK(p.resident[i] >= prev.resident[i]);
        prev = p;
    }
    CHECK(prev.launches == (int)step.size());
}

static void tinyllama()
{
    const int L = 22, E = 2048, F = 5632, KV = 256, V = 32003;
    for (int block : {kResidentBlockQ4, kResidentBlockQ8, kResidentBlockF16}) {
        const std::vector<ResidentLaunch> step = resident_step_launches(L, E, F, KV, V, block);
        CHECK(step.size() == (size_t)4 * L + 1);
        for (int l = 0; l < L; l++) {
            CHECK(step[(size_t)4 * l].family == kResidentQkv && step[(size_t)4 * l + 1].family == kResidentO);
            CHECK(step[(size_t)4 * l + 2].family == kResidentGateUp && step[(size_t)4 * l + 3].family == kResidentDown);
            for (int k = 0; k < 4; k++) CHECK(step[(size_t)4 * l + k].layer == l);
        }
        CHECK(step.back().family == kResidentHead);
        sweep(step);
        // families in ascending size: o, q|k|v, down, gate|up, lm_head -- a budget of all o and one more byte holds exactly the 22 o
        const ResidentPlan o_only = resident_plan(step, 22 * step[1].bytes + 1);
        CHECK(o_only.launches == 22 && count_family(step, o_only, kResidentO) == 22);
        // ... and one that splits q|k|v keeps its first layers
        const ResidentPlan split = resident_plan(step, 22 * step[1].bytes + 5 * step[0].bytes + 7);
        CHECK(split.launches == 27 && count_family(step, split, kResidentQkv) == 5);
        for (int l = 0; l < L; l++) CHECK(split.resident[(size_t)4 * l] == (l < 5 ? 1 : 0));
    }
    // q4: the bytes of DESIGN.md's table, and the plan at 192 MiB
    const std::vector<ResidentLaunch> q4 = resident_step_launches(L, E, F, KV, V, kResidentBlockQ4);
    CHECK(q4[0].bytes == 2949120 && q4[1].bytes == 2359296 && q4[2].bytes == 12976128 && q4[3].bytes == 6488064 && q4.back().bytes == 36867456);
    const ResidentPlan p = resident_plan(q4, 192ll << 20);
    CHECK(p.launches == 57);
    CHECK(count_family(q4, p, kResidentO) == 22 && count_family(q4, p, kResidentQkv) == 22 && count_family(q4, p, kResidentDown) == 13);
    CHECK(count_family(q4, p, kResidentGateUp) == 0 && count_family(q4, p, kResidentHead) == 0);
    for (int l = 0; l < L; l++) CHECK(p.resident[(size_t)4 * l + 3] == (l < 13 ? 1 : 0));
    CHECK(p.bytes == 22ll * 2359296 + 22ll * 2949120 + 13ll * 6488064);      // 201 129 984
    CHECK(p.bytes == 201129984ll && p.bytes <= (192ll << 20));
}

static void toy()
{
    // two layers, hand-made sizes with ties across families and layers
    std::vector<ResidentLaunch> step = {
        {kResidentQkv, 0, 300}, {kResidentO, 0, 200}, {kResidentGateUp, 0, 900}, {kResidentDown, 0, 300},
        {kResidentQkv, 1, 300}, {kResidentO, 1, 200}, {kResidentGateUp, 1, 900}, {kResidentDown, 1, 300},
        {kResidentHead, 2, 5000},
    };
    sweep(step);
    ResidentPlan p = resident_plan(step, 199);
    CHECK(p.launches == 0);
    p = resident_plan(step, 200);
    CHECK(p.launches == 1 && p.resident[1] == 1);                         // layer 0's o before layer 1's
    p = resident_plan(step, 400 + 300 + 299);
    CHECK(p.launches == 3 && p.resident[1] && p.resident[5] && p.resident[0] && !p.resident[3] && !p.resident[4] && !p.resident[7]);
    p = resident_plan(step, 400 + 900);
    CHECK(p.launches == 5 && p.resident[0] && p.resident[3] && p.resident[4] && !p.resident[7] && p.bytes == 1300);   // ties: step order
    // the first launch that does not fit ends the selection: 899 bytes are left, a 900-byte launch is next -- nothing else is tried
    p = resident_plan(step, 400 + 1200 + 899);
    CHECK(p.launches == 6 && p.bytes == 1600 && !p.resident[2] && !p.resident[6]);
    // one large launch first in step order does not block smaller ones behind it
    std::vector<ResidentLaunch> big_first = {{kResidentHead, 0, 1000}, {kResidentO, 0, 10}, {kResidentO, 1, 10}};
    p = resident_plan(big_first, 25);
    CHECK(p.launches == 2 && !p.resident[0] && p.resident[1] && p.resident[2]);
    // an empty list
    p = resident_plan(std::vector<ResidentLaunch>{}, 100);
    CHECK(p.launches == 0 && p.bytes == 0 && p.resident.empty());
    // the decoder's own traffic comes off the setting first; never below zero
    CHECK(resident_budget(192ll << 20, 24510464, 600000) == (192ll << 20) - 24510464 - 600000);
    CHECK(resident_budget(1000, 2000, 0) == 0 && resident_budget(0, 0, 0) == 0 && resident_budget(1000, -5, -5) == 1000);
}

int main()
{
    tinyllama();
    toy();
    std::printf("host_resident_plan ok\n");
    return 0;
}
