// host_shift_plan.cpp -- host/shift_plan.h alone, under ASan + UBSan (tests/test_ctx_shift_cpu.py): the plan over a grid, phi and
// the ids against their definitions written out, shifts chained until a long generation ends.
#include "../tinyllama.cpp_amd/host/shift_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace gten;

#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

int main()
{
    long plans = 0, due = 0;
    for (int max_ctx : {1, 2, 3, 7, 64, 128, 2048})
        for (int keep : {-1, 0, 1, 4, 63, 64, 2047, 2048})
            for (int drop : {-1, 0, 1, 8, 60, 2048})
                for (int rows : {-1, 0, 1, max_ctx - 1, max_ctx, max_ctx + 1})
                    for (int extra : {-1, 0, 1, 5}) {
                        const int n_ids = rows + extra;
                        ShiftPlan p;
                        const bool ok = shift_plan(n_ids, rows, max_ctx, keep, drop, &p);
                        const int d = drop > 0 ? drop : ((max_ctx - keep) / 2 > 1 ? (max_ctx - keep) / 2 : 1);
                        const bool want = rows >= 0 && extra >= 0 && rows <= max_ctx && keep >= 0 && drop >= 0 && (long long)keep + d <= max_ctx;
                        CHECK(ok == want);
                        if (!ok) continue;
                        plans++;
                        CHECK(p.due == (rows == max_ctx ? 1 : 0) && p.keep == keep);
                        if (p.due) {
                            due++;
                            CHECK(p.drop == d && p.rows == rows - d && p.n_ids == n_ids - d && p.keep + p.drop <= rows && p.drop >= 1);
                        } else {
                            CHECK(p.drop == 0 && p.rows == rows && p.n_ids == n_ids);
                        }
                    }
    CHECK(plans > 100 && due > 20);
    // phi and the ids: position p of the old sequence holds the id that position phi(p) of the new one holds, outside the dropped rows
    for (int n : {1, 5, 64, 300})
        for (int keep = 0; keep <= n; keep += (n > 16 ? 7 : 1))
            for (int drop = 1; keep + drop <= n; drop += (n > 16 ? 11 : 1)) {
                std::vector<int> ids((size_t)n + 1), old;
                for (int i = 0; i <= n; i++) ids[(size_t)i] = 1000 + i;
                old = ids;
                const int left = shift_ids(ids.data(), n + 1, keep, drop);
                CHECK(left == n + 1 - drop);
                for (int p = 0; p <= n; p++) {
                    const int q = shift_phi(p, keep, drop);
                    CHECK(q >= 0 && q < left);
                    if (p < keep || p >= keep + drop) CHECK(ids[(size_t)q] == old[(size_t)p]);
                    else CHECK(q == keep);
                }
                for (int p = 1; p <= n; p++) CHECK(shift_phi(p, keep, drop) >= shift_phi(p - 1, keep, drop));        // monotone
            }
    // a long generation: ids grow by one per step, the window never overflows, every id is accounted for
    for (int max_ctx : {8, 64})
        for (int keep : {0, 4})
            for (int drop : {0, 1, 3}) {
                int n_ids = 3, rows = 2, shifts = 0;
                long dropped = 0;
                for (int step = 0; step < 1000; step++) {
                    ShiftPlan p;
                    CHECK(shift_plan(n_ids, rows, max_ctx, keep, drop, &p));
                    if (p.due) { shifts++; dropped += p.drop; n_ids = p.n_ids; rows = p.rows; }
                    CHECK(rows < max_ctx);
                    rows++;                                  // the step writes row `rows` and yields one more id
                    n_ids++;
                }
                CHECK(shifts > 0 && n_ids + dropped == 3 + 1000 && n_ids == rows + 1);
            }
    CHECK(shift_drop(10, 0, 0) == 5 && shift_drop(10, 9, 0) == 1 && shift_drop(10, 4, 3) == 3 && shift_drop(2048, 64, 0) == 992);
    CHECK(shift_ok(10, 9, 0) && !shift_ok(10, 10, 0) && !shift_ok(10, 8, 3) && shift_ok(10, 7, 3) && !shift_ok(0, 0, 0));
    std::printf("host_shift_plan ok (%ld plans, %ld due)\n", plans, due);
    return 0;
}
