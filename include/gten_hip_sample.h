/*
 * gten_hip_sample.h -- top-k sampling with a temperature on the device, exported by libgten_hip.so beside
 * include/gten_hip.h (same conventions: device pointers unless the name ends in _host, 0 on success, otherwise a code
 * with gten_hip_last_error()).
 *
 * The contract.  A request is (top_k, temp, seed, stream).  The id that will sit at sequence position p
 * comes from the logits row x that the step for row p-1 produced:
 *   1. candidates C = the min(top_k, n_vocab) largest x_j, ties at the k-th value to the lower index;
 *   2. g_j = -log(-log(u_j)), u_j = f32((w >> 8) + 0.5) * 2^-24 capped at 1 - 2^-24, where
 *      w = Philox4x32-10(counter = (j, p, stream, 0), key = (seed & 0xffffffff, seed >> 32)) word 0;
 *   3. id = argmax over j in C of (x_j - max x) / temp + g_j in f32, the lower index winning ties.
 * top_k == 0 is greedy (strict '>', first maximum); top_k == 1 gives the same ids at any temperature.  temp must be
 * finite and > 0 when top_k >= 1, and top_k >= 0.
 */
#ifndef GTEN_HIP_SAMPLE_H
#define GTEN_HIP_SAMPLE_H

#include <stdint.h>

#include "gten_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sequence `seq` of a decoder samples from now on with this request (top_k = 0: greedy again).  Ordered on the library
 * stream before the decoder's later steps.  While no sequence of the decoder samples, its step is exactly the greedy one;
 * once one does, every step ends in the sampler (greedy sequences keep the argmax rule).  The position p is the step's n,
 * so the ids depend on the logits and on (seed, stream) only: not on the slot, the lane or the admission schedule.
 * Decoders created with the persistent step (gten_hip_set_decode_persistent) refuse top_k >= 1. */
int gten_hip_decoder_set_sampling(gten_hip_decoder* dec, int seq, int top_k, float temp, uint64_t seed, uint32_t stream);

/* The same kernel as an operator: row r of `logits` (f32, row r at logits + r * row_stride elements; a stride of 0 draws
 * every row from one vector) is sampled with top_k_host[r], temp_host[r], stream_host[r] at position_host[r]; its id goes
 * to out[r] (device).  n_vocab in [1, 65535].  Waits for the stream. */
int gten_hip_sample_rows(const float* logits, int n_rows, int n_vocab, long long row_stride, const int32_t* top_k_host,
                         const float* temp_host, uint64_t seed, const uint32_t* stream_host, const int32_t* position_host,
                         int32_t* out);

#ifdef __cplusplus
}
#endif
#endif
