/*
 * gten_hip_stoptext.h -- SEARCH automata over bytes expanded over the vocabulary on the device: stop strings given as text.
 * Exported by libgten_hip.so beside include/gten_hip_regex.h, whose conventions, vocabulary format (bytes[] + offsets[n_vocab + 1])
 * and byte automaton format (next256 u16 [Sb][256], accept u8 [Sb], state 0 the start) it shares.  DESIGN.md §3.21.
 *
 * The contract.  A search automaton looks for something in the text and bans nothing on the way.  Its Sb byte states become token
 * states [base, base + Sb] of a pool, always Sb + 1 of them; base + Sb is the HIT state, FINAL, whose row is all DEAD, and the flags of
 * the others are 0.  For s < Sb and id i:
 *   an empty piece stays: next[base + s][i] = base + s (ids beyond the tokenizer, control ids, eos: nothing is banned);
 *   a non-empty piece walks its bytes from s: base + Sb if the state after ANY byte is accepting, else base + the last state;
 *   an entry >= Sb of next256 reads as "no edge" and makes the entry DEAD (a built automaton has none).
 * The rows of accepting byte states are written by the same rule and are unreachable.  host/regex_build.h states the same in plain
 * C++ (search_expand); the kernel is held to it byte for byte.
 */
#ifndef GTEN_HIP_STOPTEXT_H
#define GTEN_HIP_STOPTEXT_H

#include <stddef.h>
#include <stdint.h>

#include "gten_hip_regex.h"

/* how a byte automaton of a part becomes token states: gten_hip_fsm_expand's rule, or the one above */
#define GTEN_HIP_FSM_PART_MATCH 0
#define GTEN_HIP_FSM_PART_SEARCH 1

#ifdef __cplusplus
extern "C" {
#endif

/* gten_hip_fsm_part with the rule its byte automaton is expanded by.  mode MATCH: count == n_byte_states + (eos >= 0).  mode SEARCH:
 * count == n_byte_states + 1 and eos == -1.  A range of host rows (rows_host != NULL) has mode MATCH. */
typedef struct {
    int first, count;
    const uint16_t* rows_host;
    const uint16_t* next256_host;
    const uint8_t* accept_host;
    int n_byte_states;
    int eos;
    int mode;
} gten_hip_fsm_part_ex;

/* Writes rows [base, base + n_byte_states] of next_dev (u16 [n_states][n_vocab]) and the same entries of flags_dev by the contract
 * above, all on the device; asynchronous on the library's stream.  The arguments are gten_hip_fsm_expand's without eos, and so are the
 * guarantees: offsets outside [0, n_bytes] read as "empty piece", automaton entries >= n_byte_states as "no edge", so no input makes
 * the kernel read or write out of bounds.  Rows outside the range are not touched. */
int gten_hip_fsm_expand_search(uint16_t* next_dev, uint8_t* flags_dev, int n_states, int n_vocab, int base, const uint8_t* bytes, long long n_bytes,
                               const int32_t* offsets, const uint16_t* next256, const uint8_t* accept, int n_byte_states);

/* gten_hip_decoder_set_fsm_parts for parts that name their mode; gten_hip_decoder_set_fsm_parts is this call with every part in mode
 * MATCH.  The finished pool is checked on the device as there (gten_hip_fsm_check_dev: the HIT state is final, every other row of a
 * search range allows ids) before the decoder adopts it. */
int gten_hip_decoder_set_fsm_parts_ex(gten_hip_decoder* dec, int n_states, const uint8_t* flags_host, const gten_hip_fsm_part_ex* parts, int n_parts);

#ifdef __cplusplus
}
#endif
#endif
