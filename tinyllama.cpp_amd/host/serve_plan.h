// serve_plan.h -- what the serving queue (host/serve.h) DECIDES: which queue items a batch of prompts takes, which
// free slots fill first, when the tail's emptiest lane moves, how long a slice is.  Device-free, like session_plan.h: integers in,
// integers out, nothing outside the result is touched; tests/host_serve_plan.cpp runs every branch on the CPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

namespace gten {

// ids in all (prompt included) that an item of P ids may reach: the queue's max_tokens, the context, and -- max_new > 0 -- P + max_new
inline int serve_limit(int P, int max_tokens, int n_ctx, int max_new)
{
    return std::min(std::min(max_tokens, n_ctx), max_new > 0 ? P + max_new : n_ctx);
}

// steps of the next slice: `slice`, cut only when EVERY live slot ends earlier (a slot whose run ends inside the slice repeats its
// last step until the slice is over)
inline int slice_steps(int slice, int longest_remaining) { return std::min(std::max(slice, 1), longest_remaining); }

// free slots in the order they are filled: slots of lanes that already run first (a lane without a live slot sits a
// run out, so a half-empty queue should occupy as few lanes as possible), then by index.  is_free(q): slot q holds no job.
template <class IsFree>
std::vector<int> free_slot_order(int n_slots, int lane_rows, int n_lanes, IsFree is_free)
{
    std::vector<int> busy((size_t)n_lanes, 0), fq;
    for (int q = 0; q < n_slots; q++)
        if (!is_free(q)) busy[(size_t)(q / lane_rows)]++;
    for (int pass = 0; pass < 2; pass++)
        for (int q = 0; q < n_slots; q++)
            if (is_free(q) && (busy[(size_t)(q / lane_rows)] > 0) == (pass == 0)) fq.push_back(q);
    return fq;
}

// THE TAIL: the lane whose sequences move -- the emptiest occupied one, the lowest index on a tie -- when the n_live live
// sequences would fit into fewer lanes than they occupy; -1: they stay where they are
inline int tail_lane_to_move(const std::vector<int>& live_per_lane, int lane_rows, int n_live)
{
    int occupied = 0, emptiest = -1;
    for (int g = 0; g < (int)live_per_lane.size(); g++)
        if (live_per_lane[(size_t)g] > 0) { occupied++; if (emptiest < 0 || live_per_lane[(size_t)g] < live_per_lane[(size_t)emptiest]) emptiest = g; }
    return occupied > (n_live + lane_rows - 1) / lane_rows ? emptiest : -1;
}

constexpr int kServeMinRows = 16;         // (GTEN_MFMA_MIN_ROWS: the shortest prompt that is a segment of the row matrix)

// one queue item as take_batch sees it
struct ServeItem {
    int P = 0;                // its ids (a session item: history + turn)
    int group = -1;           // its sample group (-1: none)
    bool session = false;     // decodes on its session's own cache set: needs no free set (and belongs to no group)
    int ctx = 0;              // > 0: a continued session item, rows [0, ctx) of its set stay ...
    int seg_rows = 0;         // ... and its segment occupies this many rows of the matrix
    int rows = 0;             // rows of the matrix it costs when it is computed (seg_rows where continued; behind a shared prefix: its own rows only)
    int limit = 0;            // serve_limit
};

// one batch of prompts: items [from, next) of the queue are consumed
struct ServeBatch {
    std::vector<int> js, limits, copy_of, ctx_of;     // per item taken: queue index, limit, the k of the item it is a copy of (-1: computed), rows kept
    std::vector<int> passed;                          // consumed without being taken: no room to generate (P >= limit), returned as they came
    int computed = 0, continued = 0, plain = 0;       // of js: prompt passes; continued segments (among the computed); items that take a set out of the pool
    size_t next = 0;
};

// The next prompts of the queue for ONE row matrix.  ITEMS: as many as there are free sets (`room`; a session item needs none);
// COMPUTED prompts: pre_max -- `cap` > 0 under a fixed schedule, whichever is smaller -- and pre_rows rows in all.  Consecutive
// items of one sample group hold the same prompt: the first one taken IN THIS CALL is computed (the lead), those behind it are
// copies, which cost neither a prompt pass nor rows -- they are still taken when the computed prompts have reached their bound, and a
// group cut by `room` goes on as a later batch's group with a lead of its own.  A prompt under kServeMinRows ids (or !batched: a
// configuration the segmented call does not compute) ends the batch without being consumed: it goes one by one.
// describe(j) -> ServeItem; it is asked once per item looked at, in queue order.
template <class Describe>
ServeBatch take_batch(size_t next, size_t n_items, int room, int cap, bool batched, int pre_max, int pre_rows, Describe describe)
{
    ServeBatch b;
    const int max_computed = std::min(pre_max, cap > 0 ? cap : pre_max);
    int rows = 0;
    int lead_k = -1, lead_group = -1;                                // this call's computed member of the group being taken
    while (next < n_items) {
        const int j = (int)next;
        const ServeItem it = describe(j);
        if (!it.session && b.plain == room) break;                   // (a session item needs no free set)
        if (!batched || it.P < kServeMinRows) break;                 // (short prompt: one by one)
        const int gid = it.session ? -1 : it.group;
        const bool copy = gid >= 0 && gid == lead_group && lead_k >= 0;
        const int cost = copy ? 0 : it.rows;
        if (!copy && (rows + cost > pre_rows || b.computed == max_computed)) break;
        next++;
        if (it.P >= it.limit) { b.passed.push_back(j); continue; }   // no room to generate: returned as is (a session stays as it is)
        if (!copy) { lead_group = gid; lead_k = (int)b.js.size(); b.computed++; }
        b.js.push_back(j); b.limits.push_back(it.limit); rows += cost; b.copy_of.push_back(copy ? lead_k : -1); b.ctx_of.push_back(it.ctx);
        if (!it.session) b.plain++;
        if (it.ctx > 0) b.continued++;
    }
    b.next = next;
    return b;
}

} // namespace gten
