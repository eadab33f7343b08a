/*
 * gten_hip_bias.h -- constrained generation on the device: per-sequence token bias tables, exported by libgten_hip.so
 * beside include/gten_hip_sample.h (same conventions: device pointers unless the name ends in _host, 0 on success,
 * otherwise a code with gten_hip_last_error()).
 *
 * The contract (it amends §3.7 only where a table is bound).  A decoder owns GTEN_HIP_BIAS_TABLES bias
 * tables, each a dense f32 row of n_vocab entries in HBM (all zero until written).  A table entry is finite with
 * |b| <= 1e30, or -inf: banned.  A sequence's request gains (table, until).  For the id that will sit at position p, drawn
 * from the logits row x, when the sequence has a table b and (until == 0 or p < until):
 *   1. y_j = x_j + b_j, one f32 add;
 *   2. the draw is that of §3.7 with y in place of x everywhere: the candidates, the maximum, (y_j - max y) / temp + g_j;
 *   3. an id with y_j = -inf is never chosen;
 *   4. with top_k larger than the number of ids above -inf, every such id is a candidate;
 *   5. top_k == 0 is the greedy rule over y (strict '>', first maximum).
 * Otherwise the draw is §3.7's, untouched.  The noise stays keyed by (j, p, stream, seed): the ids depend on the logits,
 * the table and the request only -- not on the slot, the lane or the schedule.
 */
#ifndef GTEN_HIP_BIAS_H
#define GTEN_HIP_BIAS_H

#include <stdint.h>

#include "gten_hip_sample.h"

#define GTEN_HIP_BIAS_TABLES 16
#define GTEN_HIP_BIAS_MAX 1e30f

#ifdef __cplusplus
extern "C" {
#endif

/* Table `table` of the decoder becomes: `fill` for every id, then values_host[i] for id ids_host[i], i < n (n may be 0).
 * fill = 0 with a few pairs is a logit bias / a ban list; fill = -inf with pairs of value 0 allows only those ids.
 * Refused with a code -- the table keeps its previous contents --: a table outside [0, GTEN_HIP_BIAS_TABLES), a NaN, a +inf
 * or a finite value beyond GTEN_HIP_BIAS_MAX, an id outside [0, n_vocab), a repeated id, every id banned, a decoder created
 * with the persistent step.  Ordered on the library stream before the decoder's later steps: a table may be rewritten
 * between two steps, and the next step draws with the new contents. */
int gten_hip_decoder_set_bias_table(gten_hip_decoder* dec, int table, const int32_t* ids_host, const float* values_host, int n, float fill);

/* Sequence `seq` draws under table `table` from now on, for the ids at positions < until (until == 0: at every position);
 * table = -1 clears it.  The binding is part of the sequence's request beside gten_hip_decoder_set_sampling's, which leaves
 * it alone.  While no sequence of the decoder samples or is bound, its step is exactly the greedy one; once one does or is,
 * every step ends in the sampler launch, where a greedy sequence with a table takes the argmax over y.  Decoders created
 * with the persistent step refuse a table. */
int gten_hip_decoder_set_seq_bias(gten_hip_decoder* dec, int seq, int table, int until);

/* gten_hip_sample_rows on y = x + b: row r's bias is the f32 row at bias + r * bias_stride elements (a stride of 0: one row
 * for all).  The entries follow the table rules above and at least one of a row must be above -inf (not checked: the rows
 * are on the device).  This is also what draws a prompt's first id under a table. */
int gten_hip_sample_rows_biased(const float* logits, int n_rows, int n_vocab, long long row_stride, const float* bias, long long bias_stride,
                                const int32_t* top_k_host, const float* temp_host, uint64_t seed, const uint32_t* stream_host,
                                const int32_t* position_host, int32_t* out);

/* *n_tables = GTEN_HIP_BIAS_TABLES; table_host / until_host (each [n_seq] or NULL): every sequence's binding (-1: none);
 * *table_row (may be NULL): the device address of table `table`'s row (NULL while the decoder has no tables yet, or for a
 * table outside the range) -- what gten_hip_sample_rows_biased takes as `bias` for a prompt's first id. */
int gten_hip_decoder_bias_info(gten_hip_decoder* dec, int* n_tables, int32_t* table_host, int32_t* until_host, int table, const float** table_row);

#ifdef __cplusplus
}
#endif
#endif
