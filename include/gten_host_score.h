/*
 * gten_host_score.h -- scoring given token ids with the model: per-position log-probabilities, ranks and the logits of
 * every row, exported by libgten_host.so beside include/gten_host.h (host pointers, 0 on success, < 0 on bad arguments
 * with nothing launched).  Device side: include/gten_hip_score.h.  DESIGN.md §3.8.
 */
#ifndef GTEN_HOST_SCORE_H
#define GTEN_HOST_SCORE_H

#include <stdint.h>

#include "gten_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rows [start_pos, n) of tokens computed exactly as gten_host_model_logits computes them (same modules, same path: the
 * block-rows prompt path, the operators, or the fused decoder for one row), then the lm_head over ALL of those rows.
 * targets[i] (host, n - start_pos ids, -1 = skip) is scored against row start_pos + i.  logprob_out / rank_out are host
 * arrays of n - start_pos entries (rank_out may be NULL).  The K / V caches end exactly as gten_host_model_logits leaves
 * them, so generation can go on from position n. */
int gten_host_model_score(gten_host_model* m, const int32_t* tokens, int n, int start_pos, const int32_t* targets,
                          float* logprob_out, int32_t* rank_out);
/* the same rows' logits, f32 [n - start_pos][n_vocab] (the lm_head of every row) */
int gten_host_model_logits_all(gten_host_model* m, const int32_t* tokens, int n, int start_pos, float* logits_out);
/* several independent texts: text k = tokens[starts[k] .. starts[k+1]), scored from position 0, targets / outputs aligned
 * with tokens.  Texts of 16..2048 ids go through the row-segment prompt path (gten_hip_set_row_segments) in groups of at
 * most 32 texts / 4096 rows that this call forms itself; other texts, or configurations where gten_hip_row_segments_ok is 0,
 * go one by one through gten_host_model_score.  A text's results do not depend on which texts share its group.  The
 * caches are unspecified afterwards. */
int gten_host_model_score_many(gten_host_model* m, const int32_t* tokens, const int32_t* starts, int n_texts,
                               const int32_t* targets, float* logprob_out, int32_t* rank_out);

#ifdef __cplusplus
}
#endif
#endif
