// capi_shift.cpp -- flat C exports of include/gten_host_shift.h: the shift plan, the cache primitives, generation past the window
// and shifted sessions.  Kept apart from capi.cpp: this is the only translation unit of the library that names the device entry
// point of include/gten_hip_shift.h (through host/generate_shift.h).
#include "../../include/gten_host_shift.h"

#include <algorithm>
#include <vector>

#include "capi_handles.h"
#include "generate_shift.h"

using namespace gten;

namespace {

constexpr unsigned kAll = kSampled | kBiased | kLogprobs | kNucleus | kPenalty | kFsm;
const gten_host_penalties kNone = {nullptr, nullptr, nullptr, nullptr, nullptr, 1.f, 0.f, 0.f, 0, 1};

thread_local const char* g_why = "";

int refuse(const char* why)
{
    g_why = why;
    return -1;
}

// the refusals that hold whatever keep is: this entry point has no outputs for records
const char* kNoRecords = "generate_shifting: log-prob records (n_top >= 0) are not carried through a shift and this entry point has no outputs for them";

} // namespace

extern "C" {

const char* gten_host_shift_last_error(void) { return g_why; }

int gten_host_shift_plan(int n_ids, int rows, int max_ctx, int keep, int drop, int* due, int* keep_out, int* drop_out, int* n_ids_after, int* rows_after)
{
    ShiftPlan p;
    if (!shift_plan(n_ids, rows, max_ctx, keep, drop, &p)) return -1;
    if (due) *due = p.due;
    if (keep_out) *keep_out = p.keep;
    if (drop_out) *drop_out = p.drop;
    if (n_ids_after) *n_ids_after = p.n_ids;
    if (rows_after) *rows_after = p.rows;
    return 0;
}

int gten_host_shift_drop(int rows, int keep, int drop) { return shift_ok(rows, keep, drop) ? shift_drop(rows, keep, drop) : -1; }

int gten_host_shift_phi(int p, int keep, int drop) { return shift_phi(p, keep, drop); }

int gten_host_model_shift(gten_host_model* m, int n_rows, int keep, int drop)
{
    g_why = "";
    if (!m) return refuse("model_shift: null model");
    if (n_rows > m->cfg.max_ctx || !shift_ok(n_rows, keep, drop)) return refuse("model_shift: keep + drop do not fit the valid rows");
    return kv_shift_sets({m->model.get()}, {n_rows}, keep, {shift_drop(n_rows, keep, drop)}, &m->shifts);
}

int gten_host_batch_shift(gten_host_batch* b, const int32_t* seqs, const int32_t* n_rows, int keep, int drop, int n)
{
    g_why = "";
    if (!b || !seqs || !n_rows || n < 1) return refuse("batch_shift: bad arguments");
    TinyLlamaBatch& batch = *b->batch;
    std::vector<char> seen((size_t)batch.n_seq(), 0);
    std::vector<TinyLlama*> sets;
    std::vector<int> rows, drops;
    for (int i = 0; i < n; i++) {
        if (seqs[i] < 0 || seqs[i] >= batch.n_seq() || seen[(size_t)seqs[i]]) return refuse("batch_shift: a sequence outside the batch, or named twice");
        if (n_rows[i] > b->cfg.max_ctx || !shift_ok(n_rows[i], keep, drop)) return refuse("batch_shift: keep + drop do not fit a sequence's valid rows");
        seen[(size_t)seqs[i]] = 1;
        sets.push_back(&batch.seq(seqs[i]));
        rows.push_back(n_rows[i]);
        drops.push_back(shift_drop(n_rows[i], keep, drop));
    }
    // (a "shares P rows" mark is this layer's promise that the set's leading rows are a prefix set's: it goes with the shift, as
    //  the decoder's side of it goes with the write)
    for (int i = 0; i < n; i++) batch.forget_share(seqs[i]);
    return kv_shift_sets(sets, rows, keep, drops, &b->shifts);
}

int gten_host_batch_kv_row_bytes(gten_host_batch* b)
{
    if (!b) return -1;
    return (int)gten_hip_row_bytes(b->cfg.adtype, b->cfg.n_embd / b->cfg.n_heads * b->cfg.n_kv_heads);
}

int gten_host_batch_kv_read(gten_host_batch* b, int seq, int layer, int row_from, int rows, void* k_out, void* v_out)
{
    g_why = "";
    if (!b || seq < 0 || seq >= b->batch->n_seq() || layer < 0 || layer >= b->cfg.n_layers || row_from < 0 || rows < 1 ||
        (long long)row_from + rows > b->cfg.max_ctx)
        return refuse("batch_kv_read: bad arguments");
    AttentionBlock& blk = b->batch->seq(seq).block(layer);
    const size_t pitch = (size_t)blk.attn.key.acv.bstride(0), rb = (size_t)gten_host_batch_kv_row_bytes(b);
    std::vector<uint8_t> stage((size_t)rows * pitch);
    void* outs[2] = {k_out, v_out};
    const void* srcs[2] = {blk.attn.key.acv.device_ptr(), blk.attn.value.acv.device_ptr()};
    for (int i = 0; i < 2; i++) {
        if (!outs[i]) continue;
        if (const int rc = gten_hip_memcpy_d2h(stage.data(), (const uint8_t*)srcs[i] + (size_t)row_from * pitch, stage.size())) return rc;
        for (int r = 0; r < rows; r++) std::copy_n(stage.data() + (size_t)r * pitch, rb, (uint8_t*)outs[i] + (size_t)r * rb);
    }
    return 0;
}

int gten_host_batch_shift_info(gten_host_batch* b, unsigned long long* shifts, unsigned long long* rows_moved, unsigned long long* rows_dropped)
{
    if (!b) return -1;
    if (shifts) *shifts = b->shifts.shifts;
    if (rows_moved) *rows_moved = b->shifts.rows_moved;
    if (rows_dropped) *rows_dropped = b->shifts.rows_dropped;
    return 0;
}

int gten_host_model_shift_info(gten_host_model* m, unsigned long long* shifts, unsigned long long* rows_moved, unsigned long long* rows_dropped)
{
    if (!m) return -1;
    if (shifts) *shifts = m->shifts.shifts;
    if (rows_moved) *rows_moved = m->shifts.rows_moved;
    if (rows_dropped) *rows_dropped = m->shifts.rows_dropped;
    return 0;
}

int gten_host_model_generate_shifting(gten_host_model* m, int32_t* tokens, int n_prompt, int max_tokens, int eos, int top_k, float temp, uint64_t seed,
                                      uint32_t stream, int table, int n_top, float top_p, float min_p, const gten_host_penalties* pen, int keep, int drop)
{
    g_why = "";
    if (!m || !tokens || n_prompt <= 0 || max_tokens <= 0 || !request_ok(top_k, temp) || !binding_ok(table, 0) || !cut_ok(top_p, min_p))
        return refuse("generate_shifting: bad arguments");
    if (n_top >= 0) return refuse(kNoRecords);
    const gten_host_penalties& p = pen ? *pen : kNone;
    if (!penalty_ok(p.rep_all, p.freq_all, p.pres_all, p.last_n_all)) return refuse("generate_shifting: bad penalties");
    Request r{top_k, temp, seed, stream, table, 0, -1, top_p, min_p, p.rep_all, p.freq_all, p.pres_all, p.last_n_all, p.count_prompt_all != 0};
    r.shift_keep = keep;
    r.shift_drop = drop;
    std::vector<int32_t> t(tokens, tokens + n_prompt);
    t.reserve((size_t)std::max(max_tokens, n_prompt));
    const char* why = nullptr;
    const int total = generate_shifting<kAll>(*m->model, t, max_tokens, eos, r, m->cfg.max_ctx, &m->shifts, &why);
    if (why) g_why = why;
    if (total > 0) std::copy(t.begin(), t.begin() + total, tokens);
    return total;
}

int gten_host_batch_generate_shifting(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int max_prompt, int max_tokens, int eos,
                                      int top_k, float temp, uint64_t seed, const uint32_t* stream, int table, int n_top, float top_p, float min_p,
                                      const gten_host_penalties* pen, int keep, int drop, int32_t* out, int32_t* n_total)
{
    g_why = "";
    if (!b || !prompts || !n_prompt || !out || !n_total || max_tokens <= 0 || max_prompt <= 0) return refuse("generate_shifting: bad arguments");
    if (n_top >= 0) return refuse(kNoRecords);
    const gten_host_penalties& p = pen ? *pen : kNone;
    const int S = b->batch->n_seq();
    std::vector<int32_t> tables((size_t)S, table);
    const Requests reqs = Requests::of(nullptr, top_k, nullptr, temp, seed, stream, table >= 0 ? tables.data() : nullptr, nullptr, nullptr, nullptr, top_p, nullptr, min_p)
                              .penalised(p.rep, p.rep_all, p.freq, p.freq_all, p.pres, p.pres_all, p.last_n, p.last_n_all, p.count_prompt, p.count_prompt_all);
    const char* why = nullptr;
    const int rc = generate_batch_shifting<kAll>(*b->batch, b->cfg.max_ctx, prompts, n_prompt, max_prompt, max_tokens, eos, reqs, keep, drop, out, n_total,
                                                 &b->shifts, &why);
    if (why) g_why = why;
    else if (rc == -1) g_why = "generate_shifting: bad arguments";
    return rc;
}

int gten_host_batch_session_shift(gten_host_batch* b, int id, int keep, int drop)
{
    g_why = "";
    if (!b || !b->batch->session_is_open(id)) return refuse("session_shift: no such open session");
    TinyLlamaBatch& batch = *b->batch;
    const int rows = batch.session_rows(id);
    if (!shift_ok(rows, keep, drop)) return refuse("session_shift: keep + drop do not fit the session's valid rows");
    const int d = shift_drop(rows, keep, drop);
    if (const int rc = kv_shift_sets({&batch.cset(batch.sess_base() + id)}, {rows}, keep, {d}, &b->shifts)) return rc;
    batch.session_shifted(id, keep, d);
    return 0;
}

} // extern "C"
