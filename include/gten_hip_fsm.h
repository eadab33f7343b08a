/*
 * gten_hip_fsm.h -- token automata on the device: stop sequences and masked grammars; exported by libgten_hip.so beside
 * include/gten_hip_penalty.h (same conventions: device pointers unless the name ends in _host, 0 on success, otherwise a code with
 * gten_hip_last_error()).
 *
 * The contract (it amends §3.7 / §3.12 / §3.14 only where a sequence is bound).  A decoder owns at most one POOL of S
 * states, built and checked on the host and copied to the device in one piece:
 *   next    u16[S][n_vocab], dense.  next[s][i] is the state after id i in state s, or GTEN_HIP_FSM_DEAD: id i is not allowed in s.
 *   flags   u8[S].  Bit 0 (GTEN_HIP_FSM_FINAL) marks a final state.
 * Several automata live in one pool as disjoint ranges of states; a sequence only names its start state.
 *
 * A bound sequence keeps its state PER POSITION in an int32 row of max_ctx + 2 entries, laid out like the result row: state[n] is the
 * state the id at position n is chosen in.  At the step for context length n, with s = state[n]:
 *   final s   the step draws exactly as an unbound sequence does and state[n + 1] = s.  The sequence has ended; the host stops
 *             reading it there, as after an eos, but KEEPS the id that entered the final state.
 *   else      the row is y_i = next[s][i] == DEAD ? -inf : p_i, p the raw row or the penalised one (§3.14: the penalty first, the
 *             mask second, so a ban stays a ban; no arithmetic touches an allowed logit).  Candidates, mx, scores, cut and draw are
 *             §3.7 / §3.12 on y with the same noise; a greedy sequence takes the first maximum of y.  Records (§3.11) stay computed
 *             from the raw row.  The thread that commits the id also writes state[n + 1] = next[s][id].
 * The state is a function of (row, n): a slot that repeats its step reads the same state[n] and rewrites the same state[n + 1], the
 * multi-step graphs advance it with no host help, and a sequence bound at `pos` never looks behind pos.
 *
 * A sequence may not have both a bias table (include/gten_hip_bias.h) and an automaton: nothing could then guarantee one id above
 * -inf.  Whichever setter would create the pair is refused.
 */
#ifndef GTEN_HIP_FSM_H
#define GTEN_HIP_FSM_H

#include <stddef.h>
#include <stdint.h>

#include "gten_hip_penalty.h"

#define GTEN_HIP_FSM_DEAD 0xFFFF
#define GTEN_HIP_FSM_FINAL 1
#define GTEN_HIP_FSM_MAX_STATES 65535
#define GTEN_HIP_FSM_MAX_BYTES (1ull << 30)     /* of `next`: a design limit, not a measurement */

/* gten_hip_fsm_check's codes */
#define GTEN_HIP_FSM_OK 0
#define GTEN_HIP_FSM_BAD_STATES 1               /* S outside [1, 65535], n_vocab < 1 or a null table */
#define GTEN_HIP_FSM_TOO_LARGE 2                /* S * n_vocab * 2 > GTEN_HIP_FSM_MAX_BYTES */
#define GTEN_HIP_FSM_BAD_ENTRY 3                /* an entry is neither below S nor DEAD */
#define GTEN_HIP_FSM_STUCK 4                    /* a non-final state has no allowed id */

#ifdef __cplusplus
extern "C" {
#endif

/* What an upload checks of a pool, on the host: one of the codes above.  It needs no device and no gten_hip_init.  *where (may be
 * NULL): the offending state, or -1. */
int gten_hip_fsm_check(const uint16_t* next_host, const uint8_t* flags_host, long long n_states, long long n_vocab, long long* where);

/* The decoder's pool becomes (next_host, flags_host) of n_states states over the decoder's n_vocab ids; (NULL, NULL, 0) drops the pool.
 * Refused with a code, and the previous pool stays, when gten_hip_fsm_check refuses it, when any sequence is bound at that moment, or
 * on a decoder created with the persistent step.  Synchronous. */
int gten_hip_decoder_set_fsm(gten_hip_decoder* dec, const uint16_t* next_host, const uint8_t* flags_host, int n_states);

/* "The id that will sit at position pos of sequence seq is chosen in `state`"; state -1 unbinds the sequence (pos is then not looked
 * at).  pos in [1, max_ctx].  The decoder's first binding allocates the per-sequence arrays and drops its captured graphs once; while
 * no sequence has ever been bound, the step launches exactly the kernels it did.  Refused: no pool, a state outside it, a sequence
 * that is bound to a bias table (and gten_hip_decoder_set_seq_bias refuses a table on a sequence bound here). */
int gten_hip_decoder_set_seq_fsm(gten_hip_decoder* dec, int seq, int state, int pos);

/* *n_states: the pool's S (0: none); state_host / pos_host ([n_seq] or NULL): every sequence's binding (-1, 0: unbound); *on: whether
 * a sequence has ever been bound; row_host (or NULL): a copy of sequence row_seq's state row, entries [row_from, row_from + row_count)
 * of its max_ctx + 2 (zeros while nobody has ever been bound); *next_dev / *flags_dev (may be NULL): the pool on the device, for the
 * row operators below. */
int gten_hip_decoder_fsm_info(gten_hip_decoder* dec, int* n_states, int32_t* state_host, int32_t* pos_host, int* on, int row_seq, int row_from,
                              int row_count, int32_t* row_host, const uint16_t** next_dev, const uint8_t** flags_dev);

/* gten_hip_decoder_slot_ids for the state rows: states [n_from, n_from + count) of sequence seq's row, n_from + count <= max_ctx + 2.
 * states_host[i] is the state the id at position n_from + i was (or will be) chosen in. */
int gten_hip_decoder_slot_states(gten_hip_decoder* dec, int seq, int n_from, int count, int32_t* states_host);

/* The row y of the contract for each of n_rows rows of logits, to y_out (device, row r at r * y_stride): row r is in state
 * state_host[r] of the pool (next, flags: DEVICE pointers, n_states states of n_vocab ids); -1, or a final state: not masked.  In front
 * of the mask row r is penalised as in gten_hip_penalize_rows (hist_offset_host NULL: no penalties).  The decoder's accessor, element
 * by element.  Synchronous. */
int gten_hip_mask_rows_fsm(const float* logits, int n_rows, int n_vocab, long long row_stride, const uint16_t* next, const uint8_t* flags, int n_states,
                           const int32_t* state_host, const int32_t* hist_host, const int32_t* hist_offset_host, const float* r_host,
                           const float* freq_host, const float* pres_host, float* y_out, long long y_stride);

/* gten_hip_sample_rows_pen (without a bias) with row r in state state_host[r]; next_state_out (device, [n_rows], may be NULL) receives
 * next[s][id] per row -- s itself for a final row, -1 for an unbound one.  The same row routine as the decoder's; it draws a prompt's
 * first id.  hist_offset_host NULL: no penalties.  Synchronous. */
int gten_hip_sample_rows_fsm(const float* logits, int n_rows, int n_vocab, long long row_stride, const uint16_t* next, const uint8_t* flags, int n_states,
                             const int32_t* state_host, const int32_t* top_k_host, const float* temp_host, uint64_t seed, const uint32_t* stream_host,
                             const int32_t* position_host, const float* top_p_host, const float* min_p_host, const int32_t* hist_host,
                             const int32_t* hist_offset_host, const float* r_host, const float* freq_host, const float* pres_host, int32_t* out,
                             int32_t* next_state_out, gten_hip_cut_info* info_out);

#ifdef __cplusplus
}
#endif
#endif
