/*
 * gten_host_stoptext.h -- stop strings given as TEXT, at the model level (libgten_host.so, host/capi_text.cpp), beside
 * include/gten_host_regex.h.  DESIGN.md §3.21.
 *
 * A set of byte strings becomes its Aho-Corasick automaton over BYTES on the host (host/stop_text_build.h) and a SEARCH range of an
 * automaton pool.  The pool keeps the byte automaton only; the decoder expands it over the vocabulary's byte strings ON THE DEVICE when
 * the pool is set (include/gten_hip_stoptext.h).  gten_host_fsm_tables shows the range through the host expansion (search_expand of
 * host/regex_build.h), which the device's is held to byte for byte.
 *
 * The byte automaton: states are the trie's nodes numbered breadth first from the root with bytes ascending (canonical: equal sets of
 * strings give equal tables); next256 is total, the goto function completed through the failure links; accept[s] = 1 where some string
 * is a suffix of the path to s.
 *
 * The token-level meaning, for Sb byte states placed at `base`: pool states [base, base + Sb], the last one the HIT state, FINAL, with
 * an all-DEAD row; the other flags are 0.  For s < Sb and id i:
 *   an empty piece stays in base + s (ids beyond the tokenizer, control ids, eos -- whatever the generation call's eos is);
 *   a non-empty piece walks its bytes from s: base + Sb if the state after any byte is accepting, else base + the last state.
 * NOTHING IS BANNED: up to the hit the ids are the unbound generation's.  The id that completes a string is kept, and the call ends
 * with ended_by 2; gten_host_stop_text_find tells where in the new text to cut.  The automaton starts at the first new id: a string
 * that straddles the prompt's end is not seen.
 *
 * Refusals: -1 bad arguments (no strings, an empty string, no vocabulary yet), -2 more than 65533 trie nodes or the pool's limits.
 * A refusal leaves the pool as it was.
 */
#ifndef GTEN_HOST_STOPTEXT_H
#define GTEN_HOST_STOPTEXT_H

#include <stdint.h>

#include "gten_host_regex.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The n strings (ptrs[k], lens[k] bytes: any byte may occur) as a search range of the pool; returns its start state.  Needs
 * gten_host_fsm_set_vocab first; gten_host_fsm_set_vocab is refused once such a range exists. */
int gten_host_fsm_add_stop_text(gten_host_fsm* f, const uint8_t* const* ptrs, const int32_t* lens, int n);

/* How many ranges of the pool are search ranges.  gten_host_model_set_fsm takes the route of parts when this or
 * gten_host_fsm_n_regex is above 0. */
int gten_host_fsm_n_search(const gten_host_fsm* f);

/* For inspection, device-free: the strings' byte automaton, next256_out u16 [cap_states][256] and accept_out u8 [cap_states].  Returns
 * the number of states (the tables are written only when it is <= cap_states) or a refusal as above. */
int gten_host_stop_text_dfa(const uint8_t* const* ptrs, const int32_t* lens, int n, uint16_t* next256_out, uint8_t* accept_out, int cap_states);

/* Where to cut, device-free: of all occurrences of any string in text[0, n_text) the one that ends first; among those that end at the
 * same byte the longest; among equal ones the lowest index.  Returns that index and sets [*begin, *end); no match returns -1 with
 * *begin = *end = n_text.  < -1: bad arguments. */
int gten_host_stop_text_find(const uint8_t* const* ptrs, const int32_t* lens, int n, const uint8_t* text, long long n_text, long long* begin,
                             long long* end);

#ifdef __cplusplus
}
#endif
#endif
