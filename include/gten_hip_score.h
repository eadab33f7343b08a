/*
 * gten_hip_score.h -- log-probabilities of given ids under f32 logits rows on the device, exported by libgten_hip.so
 * beside include/gten_hip.h (same conventions: device pointers, 0 on success, otherwise a code with
 * gten_hip_last_error()).  It shares the greedy rule of gten_hip_argmax_row (strict >, the first maximum wins).
 *
 * The contract.  Rows r in [0, n_rows), row r at logits + r * row_stride (floats), n_vocab entries x[j].
 * targets: int32 [n_rows] on the device; -1 (or any id outside [0, n_vocab)) = row not scored.
 *   logprob_out[r] = x[t] - (max + log(sum exp(x - max)))                          (0 for an unscored row)
 *   rank_out[r]    = #{j : x[j] > x[t] or (x[j] == x[t] and j < t)}                (-1 for an unscored row; may be NULL)
 *   argmax_out[r]  = the id gten_hip_argmax_row gives for that row, scored or not   (may be NULL)
 * rank 0 <=> the target is the greedy id.  NaN or +-inf in a row is outside the contract.  Asynchronous, current stream.
 * Checks: n_vocab >= 1, row_stride >= n_vocab, 1 <= n_rows <= 65535.  Rows are read with 16-byte loads when the base
 * and row_stride allow it (a stride padded to a multiple of 4 floats), element by element otherwise.
 */
#ifndef GTEN_HIP_SCORE_H
#define GTEN_HIP_SCORE_H

#include <stdint.h>

#include "gten_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int gten_hip_row_logprobs(const float* logits, int n_rows, int n_vocab, long long row_stride,
                          const int32_t* targets, float* logprob_out, int32_t* rank_out, int32_t* argmax_out);

#ifdef __cplusplus
}
#endif
#endif
