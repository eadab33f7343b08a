/* gten_hip_kvq4.h -- 4-bit head-major K / V shadows of the wide decoders (csrc/gten_kvq4_math.h,
 * csrc/gten_decode_attn_hm.h, csrc/gten_decode_kvq4.h).
 *
 * The head-major shadows of a decoder of 16+ sequences (gten_hip_set_kv_head_major in gten_hip.h) are derived data: the cache
 * rows stay the truth, the shadows are re-imported whenever a row is written.  Under this switch a decoder keeps them as
 * "Q4 of the Q8 block": every block {f16 d, int8 q[32]} of a row is stored as R(block) = {f16 d4, q4[32]}, q4 in [-7, 7]
 * (csrc/gten_kvq4_math.h defines R operation by operation) -- 36 instead of 68 bytes per (kv head, position), 9216 instead of
 * 17408 bytes per 256-position chunk, read by k_dec_attn_hm_q4.  LOSSY, hence off by default: the cached positions enter the
 * attention with 15 levels per block instead of 255; the newest position enters unrounded, and the cache rows themselves
 * keep their Q8 bytes for every other reader.  R is deterministic per block and idempotent, so a shadow built by appends and
 * one built by an import hold the same bytes, and a Q8-shadow decoder on rows rounded by gten_hip_kv_round_q4 computes what a
 * 4-bit decoder computes on the unrounded rows (tests/test_kv_q4_gpu.py holds the kernel to that, bit for bit). */
#ifndef GTEN_HIP_KVQ4_H
#define GTEN_HIP_KVQ4_H
#include "gten_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Decoders created AFTERWARDS keep 4-bit shadows (on != 0) or the Q8 shadows they always kept (0, the default).  Takes effect
 * only where a Q8 shadow would exist -- 16+ sequences, Q8 activations, the fast forms, head-major shadows on; everywhere else
 * (f16 activations, up to 8 sequences, the exact forms, head-major shadows switched off) it is without effect.  The
 * prefix shadows and group records of such a decoder are 4-bit shadows too. */
int gten_hip_set_kv_shadow_q4(int on);

/* What shadows a decoder keeps, as the pair (bits, bytes of one chunk of one matrix): (4, 9216) 4-bit, (8, 17408) Q8,
 * (8, 16384) FP8 shadows of f16 activations (gten_hip_kvfp8.h), (16, 32768) f16, (0, 0) none -- the chunk bytes tell the two
 * 8-bit forms apart; and the bytes of all shadows of its sequences together.  Any output may be null. */
int gten_hip_decoder_kv_shadow_info(gten_hip_decoder* dec, int* bits, int* chunk_bytes, unsigned long long* bytes_total);

/* R in place on every block of a view of Q8 rows (device memory): row r is the row_bytes bytes at rows + r * pitch, row_bytes a
 * multiple of 34 (whole blocks), rows and pitch multiples of 2 and pitch >= row_bytes -- the row-view contract of gten_hip.h;
 * the bytes between row_bytes and the pitch are neither read nor written.  Asynchronous on the library's stream.  Like every
 * writer it announces its range: a decoder that shadows these rows re-imports them before its next step. */
int gten_hip_kv_round_q4(void* rows, int n_rows, size_t row_bytes, size_t pitch);

/* The content of sequence seq's OWN shadow of (layer, kv: 0 = K, 1 = V) as dense Q8 rows [n_rows][n_kv_heads * 68] in HOST
 * memory: the quants and deltas of positions [0, n_rows) as the attention kernel reads them (the nibbles come back as int8 in
 * [-7, 7] under their f16 delta).  Positions the sequence reads from a shared prefix shadow are not in its own.  Waits for the
 * stream.  Refused on a decoder without 4-bit shadows. */
int gten_hip_decoder_kv_shadow_read(gten_hip_decoder* dec, int seq, int layer, int kv, int n_rows, void* out_rows);

#ifdef __cplusplus
}
#endif
#endif
