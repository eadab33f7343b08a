/*
 * gten_host_shift.h -- context shift on the host side: generation that goes on past the window, sessions that drop their oldest
 * turns, and the primitives both are made of; exported by libgten_host.so beside include/gten_host_sessions.h.  The device part is
 * include/gten_hip_shift.h, the definition DESIGN.md §3.20.
 *
 * shift(keep, drop) on a sequence whose rows [0, n) are valid (0 <= keep, keep + drop <= n): rows [0, keep) stay, rows
 * [keep, keep + drop) go, the m = n - keep - drop rows behind them slide down, every moved K row rotated back by drop positions.
 * drop == 0 asks for half of what lies behind keep, at least 1.  The ids become ids[:keep] + ids[keep + drop:], and everything
 * position-valued follows phi: phi(p) = p below keep, keep inside the dropped rows, p - drop behind them.
 *
 * Return codes: 0 (or a count); -1: bad arguments or a refusal of this layer, with a text in gten_host_shift_last_error();
 * otherwise the code of the device call that refused (gten_hip_last_error()).
 */
#ifndef GTEN_HOST_SHIFT_H
#define GTEN_HOST_SHIFT_H

#include <stdint.h>

#include "gten_host.h"
#include "gten_host_penalty.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sampled sequences draw on stream + (shifts << 24) after their shifts-th shift (the noise is keyed by position, and positions
 * repeat after a shift): streams at or above this are refused where shifting is asked for */
#define GTEN_HOST_SHIFT_STREAM_MAX (1u << 24)

/* the text of this thread's last refusal by one of the functions below ("" when there was none) */
const char* gten_host_shift_last_error(void);

/* ---- the plan (host/shift_plan.h), device-free.  A sequence holds n_ids ids, the leading `rows` of them with valid K / V rows; its
 * next step would write row `rows`.  *due = 1 when that row is max_ctx, i.e. a shift must come first; then *keep_out / *drop_out are
 * the pair that applies (drop resolved) and *n_ids_after / *rows_after the counts behind it (unchanged where nothing is due).
 * -1: no such plan (negative counts, rows > n_ids or > max_ctx, a pair that does not fit a full window). */
int gten_host_shift_plan(int n_ids, int rows, int max_ctx, int keep, int drop, int* due, int* keep_out, int* drop_out, int* n_ids_after, int* rows_after);
/* the drop that applies to `rows` valid rows (drop > 0: itself), or -1 where shift(keep, drop) is not possible on them */
int gten_host_shift_drop(int rows, int keep, int drop);
int gten_host_shift_phi(int p, int keep, int drop);

/* ---- primitives.  The caches of the model / of the named sequences (each once; n_rows[i] valid rows in seqs[i]) are shifted on
 * the device, all sequences and layers in ONE gten_hip_kv_shift call.  Only the caches change: the caller sets the sequence's
 * ids (decode_begin) and position for the steps that follow, and re-binds what it had bound by position through phi.  A decoder
 * of 16+ sequences re-imports the sequence's shadows before its next step, and a sequence that read a shared prefix, group or
 * chunk copy goes off that copy -- by the rule for every write into cache rows; a sharer is NOT kept on the copy even where
 * keep covers the shared chunks. */
int gten_host_model_shift(gten_host_model* m, int n_rows, int keep, int drop);
int gten_host_batch_shift(gten_host_batch* b, const int32_t* seqs, const int32_t* n_rows, int keep, int drop, int n);
/* the storage bytes of rows [row_from, row_from + rows) of sequence seq's K and V caches on `layer`, rows * row_bytes each
 * (row_bytes = gten_host_batch_kv_row_bytes); either output may be null */
int gten_host_batch_kv_read(gten_host_batch* b, int seq, int layer, int row_from, int rows, void* k_out, void* v_out);
int gten_host_batch_kv_row_bytes(gten_host_batch* b);
/* sequence-shifts done through this batch (primitives, generation and sessions), the rows they moved and dropped, per layer */
int gten_host_batch_shift_info(gten_host_batch* b, unsigned long long* shifts, unsigned long long* rows_moved, unsigned long long* rows_dropped);
int gten_host_model_shift_info(gten_host_model* m, unsigned long long* shifts, unsigned long long* rows_moved, unsigned long long* rows_dropped);

/* ---- generation past the window.  gten_host_model_generate_penalized / gten_host_batch_generate_penalized with a (keep, drop) pair:
 * keep < 0 is today's behaviour, byte for byte.  With keep >= 0 the sequence shifts whenever the plan says so and goes on until
 * max_tokens / eos: max_tokens and the out row may exceed max_ctx, the out row holds every id in generation order (shifting changes
 * what the model sees, never what the caller gets back).  After its s-th shift a sequence draws on stream + (s << 24), its penalty
 * window starts at phi(start).  REFUSED with keep >= 0 (-1, the text names it): a bias table, log-prob records (n_top >= 0), a
 * stream >= GTEN_HOST_SHIFT_STREAM_MAX, a pair that does not fit a full window, a prompt that fills the window. */
int gten_host_model_generate_shifting(gten_host_model* m, int32_t* tokens, int n_prompt, int max_tokens, int eos, int top_k, float temp, uint64_t seed,
                                      uint32_t stream, int table, int n_top, float top_p, float min_p, const gten_host_penalties* pen, int keep, int drop);
/* prompts [n_seq][max_prompt], out [n_seq][max_tokens], n_total [n_seq]; stream may be null (sequence q draws on stream q) */
int gten_host_batch_generate_shifting(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int max_prompt, int max_tokens, int eos,
                                      int top_k, float temp, uint64_t seed, const uint32_t* stream, int table, int n_top, float top_p, float min_p,
                                      const gten_host_penalties* pen, int keep, int drop, int32_t* out, int32_t* n_total);

/* ---- sessions (include/gten_host_sessions.h): the session's set is shifted on the device, its ids become ids[:keep] +
 * ids[keep + drop:], its rows rows - drop; a prefix mark is dropped unless keep >= prefix_rows.  The next serve_sessions turn goes
 * as a continued segment like any other (the drop that applies: gten_host_shift_drop(rows, keep, drop)). */
int gten_host_batch_session_shift(gten_host_batch* b, int id, int keep, int drop);

#ifdef __cplusplus
}
#endif

#endif
