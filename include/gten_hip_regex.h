/*
 * gten_hip_regex.h -- byte automata expanded over the vocabulary on the device; exported by libgten_hip.so beside
 * include/gten_hip_fsm.h (same conventions: device pointers unless the name ends in _host, 0 on success, otherwise a code with
 * gten_hip_last_error()).
 *
 * The contract.  A vocabulary is bytes[] plus offsets[n_vocab + 1]: id i spells bytes[offsets[i], offsets[i + 1]).
 * A byte automaton is next256 u16[Sb][256] (0xFFFF: no edge) and accept u8[Sb], state 0 the start.  With an eos id (or -1) it becomes
 * token states [base, base + Sb) of a pool in the format of include/gten_hip_fsm.h, and base + Sb, the END state, when eos >= 0:
 *   next[base + s][i] = base + delta*(s, bytes of i) when the walk survives every byte and the piece is not empty, else DEAD;
 *   an accepting state with no outgoing byte edge is FINAL;
 *   an accepting state with outgoing edges is not: its next[..][eos] = base + Sb, the END state, FINAL, whose row is all DEAD;
 *   eos is DEAD in every other state, whatever its bytes.
 * host/regex_build.h states the same in plain C++ (regex_expand); the kernel is held to it byte for byte.
 */
#ifndef GTEN_HIP_REGEX_H
#define GTEN_HIP_REGEX_H

#include <stddef.h>
#include <stdint.h>

#include "gten_hip_fsm.h"

/* bytes of token text a workgroup of the expansion stages at a time (a longer tile of pieces takes several rounds of the same code);
 * states one workgroup walks per pass over its staged tile, and states one workgroup covers in all */
#define GTEN_HIP_FSM_EXPAND_CHUNK 4096
#define GTEN_HIP_FSM_EXPAND_PASS 8
#define GTEN_HIP_FSM_EXPAND_STATES 64

#ifdef __cplusplus
extern "C" {
#endif

/* one range of the states of a pool under construction (gten_hip_decoder_set_fsm_parts): states [first, first + count) */
typedef struct {
    int first, count;
    const uint16_t* rows_host;          /* HOST u16 [count][n_vocab], entries pool states or DEAD: uploaded as they are; or NULL: */
    const uint16_t* next256_host;       /* HOST u16 [n_byte_states][256] */
    const uint8_t* accept_host;         /* HOST u8 [n_byte_states] */
    int n_byte_states;                  /* count == n_byte_states + (eos >= 0) */
    int eos;                            /* -1: none */
} gten_hip_fsm_part;

/* Writes rows [base, base + n_byte_states + (eos >= 0)) of next_dev (u16 [n_states][n_vocab]) and the same entries of flags_dev from
 * the vocabulary and the byte automaton, all on the device; asynchronous on the library's stream.  n_bytes is the length of
 * `bytes`: offsets outside [0, n_bytes] and automaton entries >= n_byte_states are read as "empty piece" and "no edge", so no input
 * makes the kernel read or write out of bounds.  Rows outside the range are not touched. */
int gten_hip_fsm_expand(uint16_t* next_dev, uint8_t* flags_dev, int n_states, int n_vocab, int base, const uint8_t* bytes, long long n_bytes,
                        const int32_t* offsets, const uint16_t* next256, const uint8_t* accept, int n_byte_states, int eos);

/* gten_hip_fsm_check on a pool that lives on the device: the same codes and the same *where.  Synchronous. */
int gten_hip_fsm_check_dev(const uint16_t* next_dev, const uint8_t* flags_dev, long long n_states, long long n_vocab, long long* where);

/* The decoder's vocabulary as byte strings (HOST pointers; offsets [n_vocab + 1], ascending from 0): uploaded once and kept until
 * the next call or the decoder's end.  (NULL, NULL) drops it. */
int gten_hip_decoder_set_vocab_bytes(gten_hip_decoder* dec, const uint8_t* bytes_host, const int32_t* offsets_host);

/* gten_hip_decoder_set_fsm for a pool given as ranges: the n_parts parts cover [0, n_states) in order without a gap.  A range of
 * host rows is uploaded as gten_hip_decoder_set_fsm uploads the whole; a byte automaton is expanded in place by
 * gten_hip_fsm_expand and never crosses the bus as a table (it needs gten_hip_decoder_set_vocab_bytes first).  flags_host
 * [n_states]: read for the host-row ranges only.  The finished pool is checked on the device (gten_hip_fsm_check_dev) before the
 * decoder adopts it.  The refusals, the "previous pool stays" rule and the dropping of captured graphs are
 * gten_hip_decoder_set_fsm's.  Synchronous. */
int gten_hip_decoder_set_fsm_parts(gten_hip_decoder* dec, int n_states, const uint8_t* flags_host, const gten_hip_fsm_part* parts, int n_parts);

#ifdef __cplusplus
}
#endif
#endif
