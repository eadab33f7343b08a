/*
 * gten_host_fsm.h -- token automata at the model level (libgten_host.so, host/capi_fsm.cpp), beside include/gten_host_penalty.h: stop
 * sequences and constrained choices, and whatever automaton a caller builds itself.  The rule is the device's (include/gten_hip_fsm.h,
 * DESIGN.md §3.15): a sequence bound to a state of the decoder's pool may only draw ids its state allows, its state advances on the
 * device with every id, and the id that enters a final state ends the sequence and is kept.
 *
 * The builders (gten_host_fsm_*, host/fsm_build.h) need no device.  A pool is made for one vocabulary size, automata are appended to it
 * as disjoint ranges of states, each call returning its start state (>= 0) or a refusal: -1 bad arguments (an empty sequence, an id
 * outside the vocabulary, ...), -2 the pool would pass 65535 states or GTEN_HIP_FSM_MAX_BYTES, -3 a choice is a prefix of another.
 * A refusal leaves the pool as it was.
 *
 * Each generation call carries the full request of include/gten_host_penalty.h plus a start state per item (-1: not bound) and
 * writes ended_by per item: 0 its length or the context, 1 the eos id, 2 a final state.  A bound item may not name a bias table.
 * Host pointers throughout; 0 / a count on success, < 0 on bad arguments or the device library's refusal (gten_hip_last_error).
 */
#ifndef GTEN_HOST_FSM_H
#define GTEN_HOST_FSM_H

#include <stdint.h>

#include "gten_host_penalty.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gten_host_fsm gten_host_fsm;

gten_host_fsm* gten_host_fsm_create(int n_vocab);
void gten_host_fsm_free(gten_host_fsm* f);

/* The n id sequences ids[offsets[k], offsets[k + 1]) (offsets: n + 1 ascending, the first 0) as an Aho-Corasick automaton that bans
 * nothing: walking any ids from the returned start state is in a final state exactly from the first position on at which one of the
 * sequences ends.  Empty sequences are refused. */
int gten_host_fsm_add_stop(gten_host_fsm* f, const int32_t* ids, const int32_t* offsets, int n);

/* The n choices as a trie: only its edges are allowed, and the last id of a choice enters a final state.  A choice that is empty, or a
 * prefix of another (or equal to one), is refused. */
int gten_host_fsm_add_choices(gten_host_fsm* f, const int32_t* ids, const int32_t* offsets, int n);

/* The caller's own automaton (next: u16 [n_states][n_vocab], entries below n_states or 0xFFFF; flags: u8 [n_states]), relocated. */
int gten_host_fsm_add_table(gten_host_fsm* f, const uint16_t* next, const uint8_t* flags, int n_states);

int gten_host_fsm_n_states(const gten_host_fsm* f);
/* the pool's tables, valid until the next add or free; returns the number of states */
int gten_host_fsm_tables(const gten_host_fsm* f, const uint16_t** next, const uint8_t** flags);

/* The pool becomes the pool of the model's decoder / of the batch's shared decoder (f NULL: the decoder's pool is dropped).  Refused
 * (the previous pool stays): another vocabulary size, what gten_hip_fsm_check refuses, a sequence bound at that moment. */
int gten_host_model_set_fsm(gten_host_model* m, const gten_host_fsm* f);
int gten_host_batch_set_fsm(gten_host_batch* b, const gten_host_fsm* f);

/* *n_states (may be NULL): the decoder's pool; state_out / pos_out ([n_seq], 1 entry for a model; each may be NULL): every sequence's
 * binding (-1, 0: not bound).  Returns 1 when a sequence of the decoder has ever been bound, else 0. */
int gten_host_model_fsm_info(gten_host_model* m, int* n_states, int32_t* state_out, int32_t* pos_out);
int gten_host_batch_fsm_info(gten_host_batch* b, int* n_states, int32_t* state_out, int32_t* pos_out);

/* For callers that drive the steps themselves: "the id at position pos of the model's sequence / of sequence seq of the batch is chosen
 * in `state`" (-1 unbinds; gten_hip_decoder_set_seq_fsm), and entries [from, from + count) of a sequence's state row -- entry i the
 * state the id at position from + i was, or will be, chosen in. */
int gten_host_model_set_seq_fsm(gten_host_model* m, int state, int pos);
int gten_host_batch_set_seq_fsm(gten_host_batch* b, int seq, int state, int pos);
int gten_host_model_fsm_states(gten_host_model* m, int from, int count, int32_t* states_out);
int gten_host_batch_fsm_states(gten_host_batch* b, int seq, int from, int count, int32_t* states_out);
/* ... and the batch's shared decoder itself (a gten_hip_decoder*, owned by the batch), for callers that start, run and park its slots
 * with include/gten_hip.h's gten_hip_decoder_slot_* calls beside a binding. */
void* gten_host_batch_fsm_decoder(gten_host_batch* b);

/* gten_host_model_generate_penalized with the first new id chosen in state fsm_start of the decoder's pool (-1: not bound);
 * *ended_by (may be NULL) as above.  The binding is dropped afterwards. */
int gten_host_model_generate_fsm(gten_host_model* m, int32_t* tokens, int n_prompt, int max_tokens, int eos, int top_k, float temp, uint64_t seed,
                                 uint32_t stream, int table, int min_new, int n_top, float top_p, float min_p, float* logprob_out, int32_t* top_id_out,
                                 float* top_logprob_out, const gten_host_penalties* pen, int fsm_start, int32_t* ended_by);

/* gten_host_batch_generate_penalized with a start state per sequence (fsm_start [n_seq], NULL: nobody is bound); ended_by [n_seq] or
 * NULL.  Every binding is dropped afterwards, also when a call is refused. */
int gten_host_batch_generate_fsm(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int max_prompt, int max_tokens, int eos,
                                 const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed, const uint32_t* stream,
                                 const int32_t* table, const int32_t* min_new, int32_t* out, int32_t* n_total, const int32_t* n_top, int n_top_max,
                                 float* logprob_out, int32_t* top_id_out, float* top_logprob_out, const float* top_p, const float* min_p,
                                 float top_p_all, float min_p_all, const gten_host_penalties* pen, const int32_t* fsm_start, int32_t* ended_by);

/* gten_host_batch_serve_penalized with a start state per prompt (fsm_start [n_prompts], NULL: nobody), set on whichever slot takes the
 * prompt -- again, at its current position and state, when it moves -- and dropped when the queue is done; ended_by [n_prompts] or NULL. */
int gten_host_batch_serve_fsm(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int n_prompts, int max_prompt, int max_tokens,
                              int eos, int slice, int max_new, const int32_t* max_new_each, int32_t* out, int32_t* n_total, double* stats, int n_stats,
                              const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed, const int32_t* table,
                              const int32_t* min_new, const int32_t* n_top, int n_top_max, float* logprob_out, int32_t* top_id_out,
                              float* top_logprob_out, const float* top_p, const float* min_p, float top_p_all, float min_p_all,
                              const gten_host_penalties* pen, const int32_t* fsm_start, int32_t* ended_by);

#ifdef __cplusplus
}
#endif
#endif
