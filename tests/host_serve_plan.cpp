// not gpu: the serving queue's decisions (tinyllama.cpp_amd/host/serve_plan.h) on hand-written queues, built with
// -fsanitize=address,undefined (tests/test_host_sanitize_cpu.py).  No device, no model: which items a batch of prompts takes under
// its five bounds, which free slots fill first, when the tail's emptiest lane moves, how long a slice is.  Every expectation is
// what the selection loop did while it stood inside TinyLlamaBatch::serve_with.  Exits 0 when every check holds.
#include <cstdio>
#include <vector>

#include "../tinyllama.cpp_amd/host/serve_plan.h"

using namespace gten;

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) { std::fprintf(stderr, "host_serve_plan: %s failed (line %d)\n", #c, __LINE__); return 1; } \
    } while (0)

typedef std::vector<int> V;
static const int kPreMax = 32, kPreRows = 4096;      // TinyLlamaBatch's bounds

// a plain prompt of P ids that costs `rows` rows (-1: all of its own), in group g, with room for 40 new ids
static ServeItem plain(int P, int g = -1, int rows = -1)
{
    ServeItem it;
    it.P = P; it.group = g; it.rows = rows < 0 ? P : rows; it.limit = P + 40;
    return it;
}
// a session item of P ids in all of which ctx rows stay; its segment has seg_rows rows
static ServeItem sess(int P, int ctx = 0, int seg_rows = 0)
{
    ServeItem it;
    it.P = P; it.session = true; it.ctx = ctx; it.seg_rows = seg_rows; it.rows = ctx > 0 ? seg_rows : P; it.limit = P + 40;
    return it;
}
static int g_asked_wrong = 0;
static ServeBatch take(const std::vector<ServeItem>& q, size_t next, int room, int cap = 0, bool batched = true, int pre_max = kPreMax, int pre_rows = kPreRows)
{
    int asked = 0;
    const ServeBatch b = take_batch(next, q.size(), room, cap, batched, pre_max, pre_rows, [&](int j) { asked++; return q[(size_t)j]; });
    // (every item consumed was looked at once, and at most one more: the one that ended the batch)
    if (asked < (int)(b.next - next) || asked > (int)(b.next - next) + 1) g_asked_wrong++;
    return b;
}

int main()
{
    // ---- serve_limit: max_tokens, the context, and P + max_new where max_new > 0
    CHECK(serve_limit(10, 100, 64, 0) == 64 && serve_limit(10, 50, 64, 0) == 50 && serve_limit(10, 100, 64, 5) == 15);
    CHECK(serve_limit(10, 12, 64, 5) == 12 && serve_limit(60, 100, 64, 20) == 64 && serve_limit(10, 100, 64, -1) == 64);

    // ---- 1. a group of 4 with room for 3 sets: one computed, two copies of it, the fourth left as the lead of a later batch
    {
        const std::vector<ServeItem> q{plain(100, 7), plain(100, 7), plain(100, 7), plain(100, 7), plain(50)};
        ServeBatch b = take(q, 0, 3);
        CHECK(b.js == (V{0, 1, 2}) && b.copy_of == (V{-1, 0, 0}) && b.ctx_of == (V{0, 0, 0}) && b.limits == (V{140, 140, 140}));
        CHECK(b.computed == 1 && b.continued == 0 && b.plain == 3 && b.next == 3 && b.passed.empty());
        // 2. ... whose lead was taken in an earlier call: its first item in THIS call is computed, not a copy
        b = take(q, 3, 3);
        CHECK(b.js == (V{3, 4}) && b.copy_of == (V{-1, -1}) && b.computed == 2 && b.plain == 2 && b.next == 5);
        // (two groups behind each other: each has its own lead, and copy_of speaks of positions in js)
        const std::vector<ServeItem> q2{plain(30), plain(64, 1), plain(64, 1), plain(80, 2), plain(80, 2), plain(80, 2)};
        b = take(q2, 0, 16);
        CHECK(b.js == (V{0, 1, 2, 3, 4, 5}) && b.copy_of == (V{-1, -1, 1, -1, 3, 3}) && b.computed == 3 && b.plain == 6);
    }
    // ---- 3. kPreRows by cost: a prefixed prompt counts its own rows only, a continued session item its seg_rows, a copy nothing
    {
        // 3000 + 1000 (a prompt of 1500 ids behind a prefix of 500) + 96 (a session of 2000 ids that keeps 1950: 50 rows ... a segment of 96) = 4096
        const std::vector<ServeItem> q{plain(3000), plain(1500, 3, 1000), plain(1500, 3, 1000), sess(2000, 1950, 96), plain(16)};
        ServeBatch b = take(q, 0, 8);
        CHECK(b.js == (V{0, 1, 2, 3}) && b.copy_of == (V{-1, -1, 1, -1}) && b.ctx_of == (V{0, 0, 0, 1950}));    // (... and 16 more rows do not fit)
        CHECK(b.computed == 3 && b.continued == 1 && b.plain == 3 && b.next == 4);
        // one row fewer in the matrix: the session item ends the batch -- were its cost P - ctx = 50 it would fit
        b = take(q, 0, 8, 0, true, kPreMax, 4095);
        CHECK(b.js == (V{0, 1, 2}) && b.next == 3 && b.continued == 0);
        // the whole prompt's 1500 rows would not fit behind 3000: its cost is what the description says
        b = take(q, 0, 8, 0, true, kPreMax, 3999);
        CHECK(b.js == (V{0}) && b.next == 1);
        // (a first item larger than the matrix is never taken: the caller sends it one by one)
        b = take(q, 0, 8, 0, true, kPreMax, 2999);
        CHECK(b.js.empty() && b.next == 0 && b.passed.empty());
    }
    // ---- 4. computed == min(kPreMax, cap) stops computed items; copies of the current lead are still taken
    {
        const std::vector<ServeItem> q{plain(20), plain(40, 5), plain(40, 5), plain(40, 5), plain(20), plain(40, 5)};
        ServeBatch b = take(q, 0, 16, 2);                            // (a fixed schedule's cap)
        CHECK(b.js == (V{0, 1, 2, 3}) && b.copy_of == (V{-1, -1, 1, 1}) && b.computed == 2 && b.plain == 4 && b.next == 4);
        b = take(q, 0, 16, 0, true, 2);                              // (the same through kPreMax)
        CHECK(b.js == (V{0, 1, 2, 3}) && b.computed == 2 && b.next == 4);
        b = take(q, 0, 16, 64, true, 3);                             // (cap above kPreMax: kPreMax holds; item 5 is no copy, its lead is item 4)
        CHECK(b.js == (V{0, 1, 2, 3, 4}) && b.computed == 3 && b.next == 5);
        b = take(q, 0, 3, 2);                                        // (... but a copy does need a set)
        CHECK(b.js == (V{0, 1, 2}) && b.next == 3);
    }
    // ---- 5. a session item at the head with no free set is taken, a plain item in the same state is not
    {
        const std::vector<ServeItem> q{sess(64), sess(200, 150, 50), plain(64), sess(64)};
        ServeBatch b = take(q, 0, 0);
        CHECK(b.js == (V{0, 1}) && b.copy_of == (V{-1, -1}) && b.ctx_of == (V{0, 150}) && b.computed == 2 && b.continued == 1 && b.plain == 0 && b.next == 2);
        b = take(q, 2, 0);
        CHECK(b.js.empty() && b.next == 2 && b.computed == 0);
        b = take(q, 2, 1);                                           // (one set: the plain item, and the session item behind it needs none)
        CHECK(b.js == (V{2, 3}) && b.plain == 1 && b.next == 4);
        // (a session item belongs to no group, whatever its description says, and ends the group before it)
        std::vector<ServeItem> g{plain(64, 4), sess(64), plain(64, 4)};
        g[1].group = 4;
        b = take(g, 0, 8);
        CHECK(b.js == (V{0, 1, 2}) && b.copy_of == (V{-1, -1, -1}) && b.computed == 3 && b.plain == 2);
    }
    // ---- 6. a prompt under 16 ids, or an unbatched configuration, ends the batch unconsumed; P >= limit is consumed, not taken
    {
        std::vector<ServeItem> q{plain(16), plain(15), plain(64)};
        ServeBatch b = take(q, 0, 8);
        CHECK(b.js == (V{0}) && b.next == 1 && b.passed.empty());
        b = take(q, 1, 8);
        CHECK(b.js.empty() && b.next == 1);
        b = take(q, 0, 8, 0, false);
        CHECK(b.js.empty() && b.next == 0);
        q = {plain(64), plain(64), plain(64, 9), plain(64, 9), plain(64)};
        q[1].limit = 64;                                             // no room to generate
        q[2].limit = 60;                                             // ... nor for a group's first member: the next one is its lead
        b = take(q, 0, 3);
        CHECK(b.js == (V{0, 3, 4}) && b.passed == (V{1, 2}) && b.copy_of == (V{-1, -1, -1}) && b.computed == 3 && b.plain == 3 && b.next == 5);
        // (an item without room costs nothing -- no set, no row, no prompt pass -- but it is only looked at while the batch goes on)
        b = take(q, 0, 1);
        CHECK(b.js == (V{0}) && b.next == 1 && b.passed.empty());
        b = take(q, 1, 1);
        CHECK(b.js == (V{3}) && b.passed == (V{1, 2}) && b.next == 4);
        b = take(q, 1, 8, 1);                                        // (cap 1 reached by item 3: item 4 is not a copy)
        CHECK(b.js == (V{3}) && b.passed == (V{1, 2}) && b.next == 4);
        // (a copy without room behind a lead: consumed, the copies behind it go on)
        q = {plain(64, 2), plain(64, 2), plain(64, 2)};
        q[1].limit = 64;
        b = take(q, 0, 8);
        CHECK(b.js == (V{0, 2}) && b.passed == (V{1}) && b.copy_of == (V{-1, 0}) && b.computed == 1 && b.plain == 2);
    }
    // ---- 7. free_slot_order: slots of lanes that already run first, then by index
    {
        std::vector<int> job{-1, -1, -1, -1, -1, 3, -1, -1};         // 2 lanes of 4 slots, lane 1 busy
        auto is_free = [&](int q) { return job[(size_t)q] < 0; };
        CHECK(free_slot_order(8, 4, 2, is_free) == (V{4, 6, 7, 0, 1, 2, 3}));
        job = {-1, 0, -1, -1, -1, 3, -1, 5};
        CHECK(free_slot_order(8, 4, 2, is_free) == (V{0, 2, 3, 4, 6}));
        job.assign(8, -1);
        CHECK(free_slot_order(8, 4, 2, is_free) == (V{0, 1, 2, 3, 4, 5, 6, 7}));
        job.assign(8, 1);
        CHECK(free_slot_order(8, 4, 2, is_free).empty());
        CHECK(free_slot_order(8, 8, 1, [](int q) { return q % 2 == 1; }) == (V{1, 3, 5, 7}));
    }
    // ---- 8. tail_lane_to_move: nothing at exactly fitting counts; at one lane over, the emptiest occupied lane, lowest index on a tie
    {
        CHECK(tail_lane_to_move(V{3, 2}, 4, 5) == -1);               // 5 live need 2 lanes of 4, and occupy 2
        CHECK(tail_lane_to_move(V{4, 4}, 4, 8) == -1);
        CHECK(tail_lane_to_move(V{3, 1}, 4, 4) == 1);                // 4 live fit into one
        CHECK(tail_lane_to_move(V{1, 3}, 4, 4) == 0);
        CHECK(tail_lane_to_move(V{2, 2}, 4, 4) == 0);                // (a tie: `<` keeps the first)
        CHECK(tail_lane_to_move(V{4, 0}, 4, 4) == -1 && tail_lane_to_move(V{0, 1}, 4, 1) == -1);
        CHECK(tail_lane_to_move(V{4, 2, 0, 2}, 4, 8) == 1);          // 8 live in 3 lanes fit into 2: an empty lane is not the emptiest
        CHECK(tail_lane_to_move(V{4, 3, 2}, 4, 9) == -1);
        CHECK(tail_lane_to_move(V{0, 0}, 4, 0) == -1);
    }
    // ---- 9. slice_steps: the slice, at least one step, cut to the longest remaining run
    CHECK(slice_steps(8, 100) == 8 && slice_steps(8, 8) == 8 && slice_steps(8, 3) == 3 && slice_steps(0, 5) == 1 && slice_steps(-4, 5) == 1 && slice_steps(64, 1) == 1);
    CHECK(g_asked_wrong == 0);
    std::printf("host_serve_plan ok\n");
    return 0;
}
