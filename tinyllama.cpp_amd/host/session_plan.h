// session_plan.h -- which rows a conversation's next turn computes.  Device-free: integers in, integers out;
// exported as gten_host_session_plan (include/gten_host_sessions.h) and restated by tests/sessions_ref.py.
//
// A conversation holds h ids of which the leading r have valid K / V rows (r <= h: the last generated id has no row yet, and a
// truncation may have cut rows off); a turn appends n_new ids.  The turn must end with a row to take logits from, so at most
// h + n_new - 1 rows are kept:
//     ctx  = min(r, h + n_new - 1)      rows kept
//     rows = h + n_new - ctx            rows computed, >= 1
#pragma once

namespace gten {

enum SessionPath {
    kSessionWhole = 0,        // ctx == 0: the whole-prompt path
    kSessionContinued = 1,    // where prompts are processed as segments and history + turn is one the segmented path takes (>= 16
                              // ids): one segment of a continued row matrix, filled up to 16 rows where the turn computes fewer
    kSessionOneByOne = 2,     // otherwise: the set's own model object, rows [ctx, ctx + rows)
};

struct SessionPlan {
    int ctx = 0, rows = 0, path = kSessionWhole;
    int seg_rows = 0;         // continued: the rows its segment occupies in the matrix (max(rows, 16)); otherwise 0
};

constexpr int kSessionMinRows = 16;       // (GTEN_MFMA_MIN_ROWS: the shortest segment of a row matrix, and the shortest prompt that is one)

// false: no such turn (negative counts, more valid rows than ids, or nothing to compute a row from)
inline bool session_plan(int h, int r, int n_new, bool segmented, SessionPlan* out)
{
    if (h < 0 || r < 0 || r > h || n_new < 0 || h + n_new < 1) return false;
    SessionPlan p;
    p.ctx = r < h + n_new - 1 ? r : h + n_new - 1;
    p.rows = h + n_new - p.ctx;
    p.path = p.ctx == 0 ? kSessionWhole : (h + n_new >= kSessionMinRows && segmented) ? kSessionContinued : kSessionOneByOne;
    p.seg_rows = p.path == kSessionContinued ? (p.rows < kSessionMinRows ? kSessionMinRows : p.rows) : 0;
    if (out) *out = p;
    return true;
}

// valid rows after a turn that kept `total` ids in all: the last generated id has not been through the model
inline int session_rows_after(int total, int generated) { return generated >= 1 ? total - 1 : total; }

} // namespace gten
