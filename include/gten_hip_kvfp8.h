/* gten_hip_kvfp8.h -- FP8 (OCP E4M3) head-major K / V shadows of the f16 wide decoders (csrc/gten_kvfp8_math.h,
 * csrc/gten_decode_attn_hm.h, csrc/gten_decode_kvfp8.h).
 *
 * The head-major shadows of a decoder of 16+ sequences (gten_hip_set_kv_head_major in gten_hip.h) are derived data: the cache
 * rows stay the truth, the shadows are re-imported whenever a row is written.  Under this switch a decoder on f16 activations
 * keeps them as E4M3 codes, a direct cast without a scale: every element x of a row is stored as R8(x) and read as
 * R(x) = E8(R8(x)) (csrc/gten_kvfp8_math.h: nearest of the 253 finite values, ties to the even code, beyond 448 -> +-448,
 * NaN -> +0) -- 64 instead of 128 bytes per (kv head, position), 16 384 instead of 32 768 bytes per 256-position chunk, read by
 * k_dec_attn_hm_fp8.  LOSSY, hence off by default: the cached positions enter the attention with 3 mantissa bits instead of 10;
 * the newest position enters unrounded, and the cache rows themselves keep their f16 bytes for every other reader.  R is
 * deterministic per element and idempotent, and every E4M3 value is an f16 value: an f16-shadow decoder on rows rounded by
 * gten_hip_kv_round_fp8 computes what an FP8 decoder computes on the unrounded rows (tests/test_kv_fp8_gpu.py holds the kernel
 * to that, bit for bit).  Independent of gten_hip_set_kv_shadow_q4, which acts on Q8 activations only. */
#ifndef GTEN_HIP_KVFP8_H
#define GTEN_HIP_KVFP8_H
#include "gten_hip_kvq4.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Decoders created AFTERWARDS keep FP8 shadows (on != 0) or the f16 shadows they always kept (0, the default).  Takes effect
 * only where an f16 shadow would exist -- 16+ sequences, f16 activations, the fast forms, head-major shadows on; everywhere else
 * (Q8 activations, up to 8 sequences, the exact forms, head-major shadows switched off) it is without effect.  The prefix
 * shadows and group records of such a decoder are FP8 shadows too.  gten_hip_decoder_kv_shadow_info (gten_hip_kvq4.h) answers
 * bits 8 and 16 384 bytes per chunk for such a decoder. */
int gten_hip_set_kv_shadow_fp8(int on);

/* R in place on every f16 element of a view of rows (device memory): row r is the row_bytes bytes at rows + r * pitch, row_bytes a
 * multiple of 2 (whole elements), rows and pitch multiples of 2 and pitch >= row_bytes -- the row-view contract of gten_hip.h;
 * the bytes between row_bytes and the pitch are neither read nor written.  Asynchronous on the library's stream.  Like every
 * writer it announces its range: a decoder that shadows these rows re-imports them before its next step. */
int gten_hip_kv_round_fp8(void* rows, int n_rows, size_t row_bytes, size_t pitch);

/* The content of sequence seq's OWN shadow of (layer, kv: 0 = K, 1 = V) as dense f16 rows [n_rows][n_kv_heads * 64] in HOST
 * memory: positions [0, n_rows) as the attention kernel expands them.  Positions the sequence reads from a shared prefix
 * shadow are not in its own.  Waits for the stream.  Refused on a decoder without FP8 shadows (gten_hip_decoder_kv_shadow_read
 * stays the 4-bit shadows' read-back). */
int gten_hip_decoder_kv_shadow_read_fp8(gten_hip_decoder* dec, int seq, int layer, int kv, int n_rows, void* out_rows);

#ifdef __cplusplus
}
#endif
#endif
