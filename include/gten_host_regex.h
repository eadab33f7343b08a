/*
 * gten_host_regex.h -- regular expressions as token automata at the model level (libgten_host.so, host/capi_regex.cpp), beside
 * include/gten_host_fsm.h.  DESIGN.md §3.18.
 *
 * A pattern over the TEXT becomes a byte automaton on the host (host/regex_build.h: the dialect, checkable against Python's
 * re.fullmatch(pattern, text, re.ASCII), and the canonical minimal form) and a range of states of an automaton pool.  The pool keeps
 * the byte automaton only; the decoder expands it over the vocabulary's byte strings ON THE DEVICE when the pool is set
 * (include/gten_hip_regex.h), so such a range never crosses the bus as a table.  gten_host_fsm_tables / gten_host_fsm_n_states still
 * show the whole pool: the ranges are materialised by the host expansion, plain C++ with the same definition, which the device's is
 * held to byte for byte.
 *
 * The token-level meaning, for a vocabulary bytes[] + offsets[n_vocab + 1] (id i spells bytes[offsets[i], offsets[i + 1])) and a byte
 * automaton of Sb states placed at `base`:
 *   next[base + s][i] = base + delta*(s, bytes of i) when the walk survives every byte and the piece is not empty, else DEAD;
 *   an accepting state with no outgoing byte edge is FINAL: the id that enters it ends the sequence and is kept (ended_by 2);
 *   an accepting state with outgoing edges is not final: its next[..][eos] = base + Sb, the range's one END state, which is FINAL and
 *     whose row is all DEAD -- "stop here or go on" is the model's choice, made by drawing eos;
 *   eos is DEAD in every other state; with eos = -1 there is no END state and such a state ends only by length.
 * (A generation call that is itself given the same eos id sees the eos first, as always: ended_by 1, the eos not kept.)
 *
 * Refusals follow include/gten_host_fsm.h: -1 bad arguments or bad syntax, -2 too many states (65535 subset states, or the pool's
 * limits), -4 a construct the dialect leaves out.  A refusal leaves the pool as it was.
 */
#ifndef GTEN_HOST_REGEX_H
#define GTEN_HOST_REGEX_H

#include <stdint.h>

#include "gten_host_fsm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The pool's vocabulary as byte strings (offsets [n_vocab + 1], ascending from 0).  Needed before the first gten_host_fsm_add_regex;
 * refused (-1) once the pool holds a regex range. */
int gten_host_fsm_set_vocab(gten_host_fsm* f, const uint8_t* bytes, const int32_t* offsets);

/* The byte strings of ids [0, n_vocab) as the tokenizer's decode prints them: "<0xHH>" as the single byte, no dropped leading
 * space; ids beyond the tokenizer's size and the ids of empty_ids[0 .. n_empty) (NULL: 0, 1, 2 -- <unk>, <s>, </s>) are empty.
 * offsets_out [n_vocab + 1]; bytes_out holds cap bytes (may be NULL with cap 0 to ask for the size).  Returns the total number of
 * bytes (nothing is written to bytes_out when it exceeds cap), < 0 on bad arguments. */
long long gten_host_tokenizer_vocab_bytes(gten_host_tokenizer* t, int n_vocab, const int32_t* empty_ids, int n_empty, uint8_t* bytes_out, long long cap,
                                          int32_t* offsets_out);

/* The pattern (UTF-8, NUL-terminated) as a range of the pool; returns its start state.  eos: the id that ends a sequence in an
 * accepting state that could go on, or -1.  *error_offset (may be NULL): the byte offset at which a refused pattern offends, else -1.
 * An identical (pattern, eos) of the same pool returns the range it already has. */
int gten_host_fsm_add_regex(gten_host_fsm* f, const char* pattern, int eos, int* error_offset);

/* For inspection: the pattern's byte automaton, next256_out u16 [cap_states][256] (0xFFFF: no edge) and accept_out u8 [cap_states].
 * Returns the number of states (the tables are written only when it is <= cap_states) or a refusal as above. */
int gten_host_regex_byte_dfa(const char* pattern, uint16_t* next256_out, uint8_t* accept_out, int cap_states, int* error_offset);

/* How many ranges of the pool are byte automata (0: gten_host_model_set_fsm takes the table route, as it always did). */
int gten_host_fsm_n_regex(const gten_host_fsm* f);

#ifdef __cplusplus
}
#endif
#endif
