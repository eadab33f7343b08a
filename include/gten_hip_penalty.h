/*
 * gten_hip_penalty.h -- repetition, frequency and presence penalties on the ids a sequence already holds, on the device; exported by
 * libgten_hip.so beside include/gten_hip_sample.h, include/gten_hip_bias.h, include/gten_hip_logprobs.h and include/gten_hip_nucleus.h
 * (same conventions: device pointers unless the name ends in _host, 0 on success, otherwise a code with gten_hip_last_error()).
 *
 * The contract (it amends §3.7 / §3.10 / §3.12 only where a penalty is set).  A sequence's request gains
 * (r, freq, pres, start, last_n) beside what it has.  (1, 0, 0) is "no penalty": such a sequence runs exactly what it ran before and
 * produces the same ids bit for bit; start and last_n are then not looked at (they are still range-checked).
 *
 *   window    for the id that will sit at position n: positions [lo, n) of the sequence's ids,
 *             lo = max(start, last_n > 0 ? n - last_n : 0) clamped to [0, n].  start = 0 counts the prompt, start = n_prompt only
 *             what was generated; last_n = 0 is "no limit".
 *   counts    c_i = the number of window positions that hold id i.  Ids outside [0, n_vocab) are not counted (and not refused).
 *   logit     every operation rounded to f32 on its own, whatever the build's flags:
 *               c_i == 0:  p_i = x_i
 *               c_i  > 0:  u = x_i > 0 ? x_i / r : x_i * r;   t = (float)c_i * freq;   t = t + pres;   p_i = u - t
 *             (-0 and +0 are "not > 0").
 *   row       y = p, or y_i = p_i + b_i under a bias table that holds: the penalty first, the table second, so a -inf ban stays a ban.
 *   draw      candidates, mx, scores, cut and draw are §3.7 / §3.10 / §3.12 on y with the same noise.  A greedy sequence (top_k == 0)
 *             takes the first maximum of y -- so a sequence with a penalty ends its step in the sampler launch, as one with a table does.
 *   records   log-prob records (§3.11) stay computed from the raw row x.
 * The counts are integers and p_i is a function of (x_i, c_i): nothing depends on the slot, the lane, the schedule or a reduction
 * order.  A slot that repeats its step derives the same counts and rewrites the same id.
 *
 * Refused with a code: r not finite or outside [1/8, 8]; freq or pres not finite or |.| > 100; start < 0 or last_n < 0; a penalty on
 * a decoder created with the persistent step; a decoder whose max_ctx >= 65535 (a count must fit 16 bits) or whose counts do not fit
 * the workgroup's LDS beside the sampler's own.
 */
#ifndef GTEN_HIP_PENALTY_H
#define GTEN_HIP_PENALTY_H

#include <stdint.h>

#include "gten_hip_nucleus.h"

#define GTEN_HIP_PENALTY_R_MIN 0.125f
#define GTEN_HIP_PENALTY_R_MAX 8.0f
#define GTEN_HIP_PENALTY_ADD_MAX 100.0f
#define GTEN_HIP_PENALTY_HISTORY_MAX 65535      /* window positions of one row: a count fits 16 bits */

#ifdef __cplusplus
extern "C" {
#endif

/* Sequence `seq` is penalised by (r, freq, pres) over the window (start, last_n) from now on; (1, 0, 0) clears it.  The window is
 * read from the decoder's own ids of the sequence (gten_hip_decoder_set_tokens*, and what the steps commit) when a step runs: nothing
 * else has to be uploaded, before or during generation.  It is part of the sequence's request beside the other setters', which
 * leave it alone.  The decoder's first penalty allocates the per-sequence array and drops its captured graphs once; while no sequence
 * has ever set one, the step launches exactly the kernels it did. */
int gten_hip_decoder_set_penalty(gten_hip_decoder* dec, int seq, float r, float freq, float pres, int start, int last_n);

/* r_host / freq_host / pres_host / start_host / last_n_host (each [n_seq] or NULL): every sequence's penalty ((1, 0, 0, 0, 0): none);
 * *on (may be NULL): whether a sequence of the decoder has ever set a penalty. */
int gten_hip_decoder_penalty_info(gten_hip_decoder* dec, float* r_host, float* freq_host, float* pres_host, int32_t* start_host,
                                  int32_t* last_n_host, int* on);

/* The row y of the contract for each of n_rows rows of logits, to y_out (device, row r at r * y_stride).  Row r's window is given
 * whole, already cut to size by the caller: hist_host[hist_offset_host[r] .. hist_offset_host[r + 1]) (hist_offset_host: n_rows + 1
 * ascending offsets, the first 0; at most GTEN_HIP_PENALTY_HISTORY_MAX ids per row; hist_host may be NULL when there are none).
 * bias (may be NULL) as in gten_hip_sample_rows_biased.  The decoder's accessor, element by element.  Synchronous. */
int gten_hip_penalize_rows(const float* logits, int n_rows, int n_vocab, long long row_stride, const float* bias, long long bias_stride,
                           const int32_t* hist_host, const int32_t* hist_offset_host, const float* r_host, const float* freq_host,
                           const float* pres_host, float* y_out, long long y_stride);

/* gten_hip_sample_rows_cut with row r penalised by (r_host[r], freq_host[r], pres_host[r]) over its window (as above).  The same row
 * routine as the decoder's.  A row with (1, 0, 0) runs gten_hip_sample_rows_cut's code.  Synchronous. */
int gten_hip_sample_rows_pen(const float* logits, int n_rows, int n_vocab, long long row_stride, const float* bias, long long bias_stride,
                             const int32_t* top_k_host, const float* temp_host, uint64_t seed, const uint32_t* stream_host,
                             const int32_t* position_host, const float* top_p_host, const float* min_p_host, const int32_t* hist_host,
                             const int32_t* hist_offset_host, const float* r_host, const float* freq_host, const float* pres_host,
                             int32_t* out, gten_hip_cut_info* info_out);

#ifdef __cplusplus
}
#endif
#endif
