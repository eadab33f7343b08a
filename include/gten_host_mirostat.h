/*
 * gten_host_mirostat.h -- Mirostat v2 (include/gten_hip_mirostat.h) on a host model's or batch's decoder; exported by
 * libgten_host.so beside include/gten_host_fsm.h (same conventions: 0 on success, -1 for a null handle, otherwise the decoder's code
 * with gten_hip_last_error()).
 *
 * The three generation entry points are include/gten_host_fsm.h's with a Mirostat request behind their arguments: miro_tau 0 is "off"
 * (the call is then its _fsm form, id for id), otherwise 0 < tau <= 32 and 0 < eta <= 1.  A prompt's first id is drawn by
 * gten_hip_sample_rows_miro from mu = 2 tau, the decoder is bound at the next position with the mu that returns, and wherever the queue
 * sets a slot's request again -- a move between lanes in the tail included -- it rebinds at the slot's current position with the mu read
 * back.  A greedy item ignores Mirostat.  An item that carries both a cut other than (1, 0) and Mirostat is refused by name (-1, a line
 * on stderr) before any work.  No binding is left behind, whatever way a call ends.
 * The other calls set, read and clear a sequence's binding for decode steps the caller drives itself (decode_begin / decode_step).
 */
#ifndef GTEN_HOST_MIROSTAT_H
#define GTEN_HOST_MIROSTAT_H

#include <stdint.h>

#include "gten_host.h"
#include "gten_host_penalty.h"

#ifdef __cplusplus
extern "C" {
#endif

int gten_host_model_generate_mirostat(gten_host_model* m, int32_t* tokens, int n_prompt, int max_tokens, int eos, int top_k, float temp, uint64_t seed,
                                      uint32_t stream, int table, int min_new, int n_top, float top_p, float min_p, float* logprob_out,
                                      int32_t* top_id_out, float* top_logprob_out, const gten_host_penalties* pen, int fsm_start, int32_t* ended_by,
                                      float miro_tau, float miro_eta);
int gten_host_batch_generate_mirostat(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int max_prompt, int max_tokens, int eos,
                                      const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed, const uint32_t* stream,
                                      const int32_t* table, const int32_t* min_new, int32_t* out, int32_t* n_total, const int32_t* n_top, int n_top_max,
                                      float* logprob_out, int32_t* top_id_out, float* top_logprob_out, const float* top_p, const float* min_p,
                                      float top_p_all, float min_p_all, const gten_host_penalties* pen, const int32_t* fsm_start, int32_t* ended_by,
                                      const float* miro_tau, const float* miro_eta, float miro_tau_all, float miro_eta_all);
int gten_host_batch_serve_mirostat(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int n_prompts, int max_prompt, int max_tokens,
                                   int eos, int slice, int max_new, const int32_t* max_new_each, int32_t* out, int32_t* n_total, double* stats,
                                   int n_stats, const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed,
                                   const int32_t* table, const int32_t* min_new, const int32_t* n_top, int n_top_max, float* logprob_out,
                                   int32_t* top_id_out, float* top_logprob_out, const float* top_p, const float* min_p, float top_p_all, float min_p_all,
                                   const gten_host_penalties* pen, const int32_t* fsm_start, int32_t* ended_by, const float* miro_tau,
                                   const float* miro_eta, float miro_tau_all, float miro_eta_all);

/* gten_hip_decoder_set_seq_mirostat on the model's only sequence / on sequence seq of the batch: the ids from position pos on are
 * drawn under Mirostat (tau, eta), mu starting at mu_q16 (INT32_MIN: 2 * tau_q); tau == 0 unbinds. */
int gten_host_model_set_mirostat(gten_host_model* m, float tau, float eta, int32_t mu_q16, int pos);
int gten_host_batch_set_mirostat(gten_host_batch* b, int seq, float tau, float eta, int32_t mu_q16, int pos);

/* Every sequence's binding (tau_q_out / eta_q_out / pos_out: [1] for a model, [n_seq] for a batch, or NULL; zeros: unbound).  Returns 1
 * when a sequence of the decoder has ever been bound, 0 when none has, -1 on an error. */
int gten_host_model_mirostat_info(gten_host_model* m, int32_t* tau_q_out, int32_t* eta_q_out, int32_t* pos_out);
int gten_host_batch_mirostat_info(gten_host_batch* b, int32_t* tau_q_out, int32_t* eta_q_out, int32_t* pos_out);

/* gten_hip_decoder_slot_mus: entries [from, from + count) of the sequence's mu row (Q16; zeros while nobody has ever been bound). */
int gten_host_model_mirostat_mus(gten_host_model* m, int from, int count, int32_t* mus_out);
int gten_host_batch_mirostat_mus(gten_host_batch* b, int seq, int from, int count, int32_t* mus_out);

#ifdef __cplusplus
}
#endif
#endif
