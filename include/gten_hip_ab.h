/* gten_hip_ab.h: A/B controls of libgten_hip.so -- switches that select an older kernel which computes the same bytes as the
 * default one, kept to measure the two against each other and as the reference the tests hold the new kernel to. */
#pragma once

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

#ifdef __cplusplus
}
#endif
