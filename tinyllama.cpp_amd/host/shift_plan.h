// shift_plan.h -- when a sequence that has filled its window shifts, and by how much.  Device-free: integers in,
// integers out; exported as gten_host_shift_plan / gten_host_shift_phi (include/gten_host_shift.h), restated by
// tests/test_ctx_shift_cpu.py and exercised under sanitizers by tests/host_shift_plan.cpp.
//
// A sequence holds n_ids ids of which the leading `rows` have valid K / V rows (rows <= n_ids: the last generated id has no row
// yet).  Its next step writes row `rows`; there are rows [0, max_ctx).  So a shift is DUE before the step that would write row
// max_ctx, i.e. exactly when rows == max_ctx.  shift(keep, drop) keeps rows [0, keep), drops rows [keep, keep + drop) and slides
// the rest down; drop == 0 asks for half of what lies behind keep, at least 1.  The pair must be possible on a full window:
//     0 <= keep,  keep + drop <= max_ctx   (with the drop that applies: at least 1)
#pragma once

namespace gten {

struct ShiftPlan {
    int due = 0;              // 1: shift before the next step
    int keep = 0, drop = 0;   // the pair that applies (drop resolved; 0 where nothing is due)
    int n_ids = 0, rows = 0;  // ids held and valid rows after it (unchanged where nothing is due)
};

// sequence-shifts done, and the rows they moved and dropped (per layer)
struct ShiftCounts { unsigned long long shifts = 0, rows_moved = 0, rows_dropped = 0; };

// the drop that applies to `rows` valid rows: the caller's, or half of what lies behind keep (at least 1)
inline int shift_drop(int rows, int keep, int drop) { return drop > 0 ? drop : ((rows - keep) / 2 > 1 ? (rows - keep) / 2 : 1); }

// whether shift(keep, drop) is possible on `rows` valid rows (drop as the caller gave it: 0 = half)
inline bool shift_ok(int rows, int keep, int drop) { return keep >= 0 && drop >= 0 && rows >= 1 && (long long)keep + shift_drop(rows, keep, drop) <= rows; }

// false: no such plan (negative counts, more rows than ids or than the window, a pair that does not fit a full window)
inline bool shift_plan(int n_ids, int rows, int max_ctx, int keep, int drop, ShiftPlan* out)
{
    if (n_ids < 0 || rows < 0 || rows > n_ids || max_ctx < 1 || rows > max_ctx || !shift_ok(max_ctx, keep, drop)) return false;
    ShiftPlan p;
    p.n_ids = n_ids;
    p.rows = rows;
    p.keep = keep;
    if (rows == max_ctx) {
        p.due = 1;
        p.drop = shift_drop(rows, keep, drop);
        p.n_ids = n_ids - p.drop;
        p.rows = rows - p.drop;
    }
    if (out) *out = p;
    return true;
}

// where position p of the old sequence lies after shift(keep, drop): everything position-valued follows this one map
inline int shift_phi(int p, int keep, int drop) { return p < keep ? p : p < keep + drop ? keep : p - drop; }

// the ids after shift(keep, drop), in place: ids[:keep] + ids[keep + drop:]; returns the new count
inline int shift_ids(int* ids, int n_ids, int keep, int drop)
{
    for (int i = keep + drop; i < n_ids; i++) ids[i - drop] = ids[i];
    return n_ids - drop;
}

} // namespace gten
