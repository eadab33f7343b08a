/* gten_hip_ab.h: A/B controls of libgten_hip.so -- switches that select an older kernel which computes the same bytes as the
 * default one, kept to measure the two against each other and as the reference the tests hold the new kernel to. */
#pragma once

#ifdef __cplusplus
extern "C" {
#endif

/* The single-sequence attention of decoders created AFTERWARDS (d_head 64, fast forms; a decoder keeps the choice it was
 * created with): on != 0 runs round 5's k_dec_attn_one64 -- the V chunk in LDS as cache bytes, three LDS reads and a
 * dequantization per p.V term -- and 0 (the default) k_dec_attn_one64v -- each thread widens its own V row to f32 in LDS
 * once, one LDS read per term (csrc/gten_decode_attn.h).  Both write bit-identical attention partials and statistics
 * (tests/test_decode_attn_bytes_gpu.py).  Decoders of 2+ sequences and the exact forms (gten_hip_set_decode_exact) are not
 * affected. */
int gten_hip_set_decode_attn_classic(int on);

#ifdef __cplusplus
}
#endif
