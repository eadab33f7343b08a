/*
 * gten_host_embed.h -- the hidden states of texts: every row in storage form, or one pooled f32 vector per text, exported by
 * libgten_host.so beside include/gten_host.h (host pointers, 0 on success; < 0 with nothing computed and a text in
 * gten_host_embed_last_error()).  Device side: include/gten_hip_embed.h, which defines the pooling.  DESIGN.md §3.22.
 *
 * Texts: text k = tokens[starts[k] .. starts[k + 1]), starts[0] == 0, every text processed from position 0 on its own.
 * Refused: no texts, an empty text, a text over min(2048, max_ctx) ids, an id outside [0, n_vocab), a layer outside
 * [0, n_layers], an unknown pooling, a null pointer.  The model works as before after a refusal.
 *
 * Which texts share a prompt pass is gten_host_embed_plan's decision, the rule of gten_host_model_score_many: texts of
 * 16 .. 2048 ids go through the row-segment prompt path in groups of at most 32 texts / 4096 rows on a second model that aliases
 * the weights (the one score_many uses), every other text -- or all, where gten_hip_row_segments_ok is 0 -- goes alone through
 * the model's own operators.  A text's bytes do not depend on which texts share its group.
 *
 * layer: 0 or n_layers gives the model's own output, the final norm of the last block.  1 <= layer < n_layers gives the FINAL
 * NORM APPLIED TO THE OUTPUT OF BLOCK `layer` (blocks counted from 1; the logit-lens convention): the bytes a model of `layer`
 * layers with the same leading weights and the same final norm gives.  The blocks behind it are not run.
 *
 * No lm_head launch happens in either call.  What they do to the model's own K / V caches is what gten_host_model_score_many
 * does to them: the caches are unspecified afterwards (a text that goes alone overwrites rows [0, its length) of the blocks
 * that ran; grouped texts use the second model's caches).  Generation must start again from its prompt.
 *
 * One calling thread, like the rest of the library: embed_many stages its vectors in one device buffer per process (grown on
 * demand, kept until the process ends, shared by all models), and each call is synchronous -- it returns after its copy back.
 */
#ifndef GTEN_HOST_EMBED_H
#define GTEN_HOST_EMBED_H

#include <stdint.h>

#include "gten_host.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GTEN_HOST_POOL_MEAN 0   /* GTEN_HIP_POOL_MEAN */
#define GTEN_HOST_POOL_LAST 1   /* GTEN_HIP_POOL_LAST */

/* the text of the last refusal by an entry point of this header ("" after a success) */
const char* gten_host_embed_last_error(void);

/* the plan (host/embed_plan.h), device-free: group_of[k] = the group of text k, alone[g] = 1 where group g is one text that goes
 * alone (either may be NULL; both have room for n_texts entries).  Groups are numbered in the order of their first texts.
 * seg_ok: what gten_hip_row_segments_ok says for the configuration.  Returns the number of groups; -1: no texts, or a text
 * without ids. */
int gten_host_embed_plan(const int32_t* lengths, int n_texts, int seg_ok, int32_t* group_of, int32_t* alone);

/* every text's rows after the final norm, in the activation dtype's storage form (*dtype_out: GTEN_Q8 or GTEN_F16), copied to
 * rows_out: starts[n_texts] rows of gten_hip_row_bytes(dtype, n_embd) bytes each, row starts[k] + r = row r of text k. */
int gten_host_model_hidden_many(gten_host_model* m, const int32_t* tokens, const int32_t* starts, int n_texts, int layer,
                                void* rows_out, int* dtype_out);

/* the same passes; each group's rows are pooled on the device (gten_hip_pool_rows: pooling GTEN_HOST_POOL_*, normalize 0 / 1)
 * and all vectors come back in one copy at the end.  out: f32 [n_texts][n_embd]. */
int gten_host_model_embed_many(gten_host_model* m, const int32_t* tokens, const int32_t* starts, int n_texts, int pooling,
                               int normalize, int layer, float* out);

#ifdef __cplusplus
}
#endif
#endif
