/* gten_hip_ab.h: A/B controls of libgten_hip.so -- switches that select an older kernel which computes the same bytes as the
 * default one, kept to measure the two against each other and as the reference the tests hold the new kernel to. */
#pragma once

#include "gten_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The single-sequence attention of decoders created AFTERWARDS (d_head 64, fast forms; a decoder keeps the choice it was
 * created with), csrc/gten_decode_attn.h and csrc/gten_decode_attn_w.h:
 *   0 (the default)  k_dec_attn_one64w -- 512 threads in two roles: waves 0-3 carry the softmax chain (K rows, q, scores,
 *                    statistics, probabilities, p.V), waves 4-7 request the V rows, widen them to f32 in LDS beside the
 *                    chain and prepare and append the new k / v rows;
 *   1                round 5's k_dec_attn_one64 -- the V chunk in LDS as cache bytes, three LDS reads and a dequantization
 *                    per p.V term (the A/B control the tests hold the others to);
 *   2                k_dec_attn_one64v -- 256 threads; each thread widens its own V row to f32 in LDS between its score
 *                    and the chunk maximum, one LDS read per p.V term.
 * All three write bit-identical attention partials, statistics and cache rows (tests/test_decode_attn_bytes_gpu.py,
 * tests/test_decode_attn_helpers_gpu.py).  Any other value is an error.  Decoders of 2+ sequences and the exact forms
 * (gten_hip_set_decode_exact) are not affected. */
int gten_hip_set_decode_attn_classic(int v);

/* Which weights a single-sequence decoder created AFTERWARDS keeps in the memory-side cache.  Every weight request
 * of the step's W.x launches is nontemporal by default: the weights as a whole do not fit that cache, and streamed with the default
 * policy they would displace what the step re-reads.  A part of them fits, and the weights are the same from token to token: with a
 * budget of `mb` MiB the decoder takes off its own K / V rows at max_ctx and its scratch, and gives the rest to its W.x launches in
 * ascending order of their weight bytes (the smallest matrices first; ties: the earlier launch), each whole or not at all, until
 * the first one that does not fit (host/resident_plan.h).  Those launches run the same kernel with the default cache policy on
 * their weight requests -- the same bytes out, whatever the budget.  0: every request nontemporal, the A/B control.  A negative
 * value is an error.  Unset, the value is the environment's GTEN_HIP_RESIDENT_MB, else the compiled-in default.  A decoder keeps
 * the plan it was created with (its graphs are captured once); decoders of 2+ sequences and the exact forms always keep budget 0.
 * _bytes: the same setting to the byte (what a test splits a family of a small model with). */
int gten_hip_set_weight_resident_mb(int mb);
int gten_hip_set_weight_resident_bytes(long long bytes);
/* the setting a decoder created now would take, in bytes (a test puts it back with gten_hip_set_weight_resident_bytes) */
long long gten_hip_weight_resident_bytes(void);
/* what a decoder decided: how many of its W.x launches are resident and their weight bytes */
int gten_hip_decoder_resident(gten_hip_decoder* dec, int* launches, long long* bytes);
/* ... the bytes it had left for them, and what it took off the setting first (its K / V rows and scratch) */
int gten_hip_decoder_resident_budget(gten_hip_decoder* dec, long long* budget, long long* overhead);

#ifdef __cplusplus
}
#endif
