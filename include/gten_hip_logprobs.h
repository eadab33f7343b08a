/*
 * gten_hip_logprobs.h -- the log-prob of every generated id and the top-N alternatives of its step, on the device; exported by
 * libgten_hip.so beside include/gten_hip_sample.h and include/gten_hip_bias.h (same conventions: device pointers unless the
 * name ends in _host, 0 on success, otherwise a code with gten_hip_last_error()).
 *
 * The contract.  Sequence q of a decoder may ask for log-probs with n_top in [0, GTEN_HIP_LOGPROBS_TOP], or
 * -1 for off (the default).  While it asks, every decode step of q that commits an id at position p (result[p]) also commits
 * one record for p, computed from the step's RAW logits row x -- no bias table, temperature 1, the whole vocabulary:
 *   lse            = max x + log(sum_j exp(x_j - max x)), f32;
 *   logprob        = x[id] - lse, id the id this step committed (greedy, drawn, or drawn under a table);
 *   top_id[0..m)   = the m = min(n_top, n_vocab) largest x_j in descending order; -0 == +0; ties go to the lower index, at the
 *                    cut and inside the list -- exact integer facts about the row.  top_id[0] is gten_hip_argmax_row's id;
 *   top_logprob[i] = x[top_id[i]] - lse: the same lse, the same single subtraction -- where id is in the list its entry
 *                    equals logprob bit for bit;
 *   entries [m, GTEN_HIP_LOGPROBS_TOP) are id -1, logprob 0.
 * NaN or +-inf in a row is outside the contract.  The record depends on the row and the committed id only: not on the slot,
 * the lane, the schedule or on which other sequences ask.  A slot that repeats its last step rewrites the same bytes.  The
 * ids of every entry point are the same with the request on or off.
 *
 * The records of a decoder lie in one device buffer [n_seq][max_ctx + 2], indexed by position like the ids; a record is
 * GTEN_HIP_LOGPROBS_RECORD_BYTES bytes: f32 lse, f32 logprob, int32 top_id[20], f32 top_logprob[20].
 */
#ifndef GTEN_HIP_LOGPROBS_H
#define GTEN_HIP_LOGPROBS_H

#include <stdint.h>

#include "gten_hip_sample.h"

#define GTEN_HIP_LOGPROBS_TOP 20
#define GTEN_HIP_LOGPROBS_RECORD_BYTES 168

#ifdef __cplusplus
extern "C" {
#endif

/* Sequence `seq` asks for records with n_top alternatives from now on (0: only the committed id's log-prob), -1 ends the
 * request.  It is part of the sequence's request beside gten_hip_decoder_set_sampling's and gten_hip_decoder_set_seq_bias's,
 * which leave it alone.  The decoder's first request allocates the record buffer (zeroed) and drops its captured graphs once.
 * While no sequence samples, is bound or asks, the step is exactly the greedy one; otherwise it ends in the sampler launch,
 * where a greedy sequence takes the argmax rule.  Decoders created with the persistent step refuse a request. */
int gten_hip_decoder_set_logprobs(gten_hip_decoder* dec, int seq, int n_top);

/* The records of sequence `seq` at positions [n_from, n_from + count): logprob_host[count], top_id_host and top_logprob_host
 * [count][n_top] (the first n_top entries of each record; both may be NULL when n_top == 0).  Waits for the queued steps, as
 * gten_hip_decoder_slot_ids does.  A position at which the sequence committed no record while asking holds what was there
 * before (zeros after the first request).  An error while the decoder has no record buffer. */
int gten_hip_decoder_logprobs(gten_hip_decoder* dec, int seq, int n_from, int count, int n_top, float* logprob_host, int32_t* top_id_host,
                              float* top_logprob_host);

/* *top_cap = GTEN_HIP_LOGPROBS_TOP; n_top_host ([n_seq] or NULL): every sequence's request (-1: none); *records: the device
 * address of the record buffer (NULL before the first request); *seq_stride_bytes: from one sequence's records to the
 * next's; *record_bytes = GTEN_HIP_LOGPROBS_RECORD_BYTES.  Every output may be NULL. */
int gten_hip_decoder_logprobs_info(gten_hip_decoder* dec, int* top_cap, int32_t* n_top_host, const void** records, long long* seq_stride_bytes,
                                   int* record_bytes);

/* The record of rows that are already on the device: row r at logits + r * row_stride elements, ids[r] (device) the chosen
 * id (-1: none, logprob 0).  logprob_out [n_rows], top_id_out and top_logprob_out [n_rows][n_top] (entries from
 * min(n_top, n_vocab) on: -1 / 0).  Asynchronous on the current stream.  The same routine as the decoder's: bit-equal to its
 * records on the same row.  Refused: n_vocab < 1, row_stride < n_vocab, n_rows outside [1, 65535], n_top outside
 * [0, GTEN_HIP_LOGPROBS_TOP]. */
int gten_hip_row_top_logprobs(const float* logits, int n_rows, int n_vocab, long long row_stride, const int32_t* ids, int n_top, float* logprob_out,
                              int32_t* top_id_out, float* top_logprob_out);

#ifdef __cplusplus
}
#endif
#endif
