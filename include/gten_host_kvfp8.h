/*
 * gten_host_kvfp8.h -- FP8 head-major K / V shadows at the level of a batch: the rounding R over a sequence's f16 cache rows and a
 * shadow's content; exported by libgten_host.so (host/capi_kvfp8.cpp) beside include/gten_host_kvq4.h, whose
 * gten_host_batch_kv_shadow_info and gten_host_batch_kv_rows serve these shadows as well.  The device's part is
 * include/gten_hip_kvfp8.h (the switch is set there, before the batch's decoder is created); DESIGN.md 3.25.
 */
#ifndef GTEN_HOST_KVFP8_H
#define GTEN_HOST_KVFP8_H

#include "gten_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* R (csrc/gten_kvfp8_math.h) in place on cache rows [0, n_rows) of sequence seq, every layer, K and V: afterwards the rows hold what an
 * FP8 shadow holds of them.  f16 activations only.  The writes are announced, so a decoder that shadows the rows re-imports them.
 * 0, or non-zero */
int gten_host_batch_kv_round_fp8(gten_host_batch* b, int seq, int n_rows);

/* rows [0, n_rows) of sequence seq's own shadow on `layer` as dense f16 rows [n_rows][kv row bytes] (gten_host_batch_kv_read's
 * shape): k_out and v_out in host memory, either may be NULL.  Refused where the decoder keeps no FP8 shadows. */
int gten_host_batch_kv_shadow_read_fp8(gten_host_batch* b, int seq, int layer, int n_rows, void* k_out, void* v_out);

#ifdef __cplusplus
}
#endif
#endif
