/*
 * gten_host_beam.h -- beam search as a fixed-batch call, and the host's part of it without a device; exported by libgten_host.so
 * (host/capi_beam.cpp) beside include/gten_host.h.  The device's part is include/gten_hip_beam.h; DESIGN.md §3.19.
 */
#ifndef GTEN_HOST_BEAM_H
#define GTEN_HOST_BEAM_H

#include <stdint.h>

#include "gten_host.h"

#define GTEN_HOST_BEAM_MAX 8
#define GTEN_HOST_BEAM_STATE_BYTES 176
#define GTEN_HOST_BEAM_ENDED_EOS 0
#define GTEN_HOST_BEAM_ENDED_LENGTH 1

#ifdef __cplusplus
extern "C" {
#endif

/* n_prompts prompts (prompt g: tokens[starts[g] .. starts[g + 1])) x n_beams beams on sequences g * n_beams + b of the batch
 * (n_prompts * n_beams <= n_seq; the other sequences idle), at most max_new rounds, ended early once every prompt has n_beams
 * finished hypotheses.  eos -1: none.  A hypothesis' score is final = cum * (float)(1 / t^length_penalty), t its rounds.
 * Per prompt the best n_hyp[g] <= n_beams hypotheses, best first, at index (g * n_beams + i):
 *   ids_out [.][max_new] and n_ids_out [.]: the new ids (eos not stored); final_out, cum_out; ended_by_out: GTEN_HOST_BEAM_ENDED_*.
 * rounds_out (may be NULL): the rounds that ran.  0; -1: bad arguments; otherwise the device's refusal (gten_hip_last_error()). */
int gten_host_batch_beam_search(gten_host_batch* b, const int32_t* tokens, const int32_t* starts, int n_prompts, int n_beams, int max_new, int eos,
                                float length_penalty, int32_t* ids_out, int32_t* n_ids_out, float* final_out, float* cum_out, int32_t* ended_by_out,
                                int32_t* n_hyp, int* rounds_out);

/* ---- the plan (host/beam_plan.h), callable without a device */
/* w_out[max_new + 1]: w[0] = 0, w[t] = (float)(1 / t^length_penalty) */
int gten_host_beam_weights(int max_new, float length_penalty, float* w_out);
/* the ids of beam b after round t of a trellis whose round r lies at row r - 1 ([rows][GTEN_HOST_BEAM_MAX] each): out[t]; returns t,
 * or -1 where t, b or a parent lie outside the trellis */
int gten_host_beam_backtrack(const int32_t* parent, const int32_t* ids, int rows, int t, int b, int32_t* out);
/* state: the device's GTEN_HOST_BEAM_STATE_BYTES of one group; w[state.t + 1] at least.  Outputs as above for one prompt
 * ([n_beams][max_new] ids); returns the number of hypotheses, or -1 */
int gten_host_beam_finalize(const void* state, const int32_t* parent, const int32_t* ids, int rows, int n_beams, const float* w, int max_new,
                            int32_t* ids_out, int32_t* n_ids_out, float* final_out, float* cum_out, int32_t* ended_by_out);

#ifdef __cplusplus
}
#endif
#endif
