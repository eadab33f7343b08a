/*
 * gten_host_kvq4.h -- 4-bit head-major K / V shadows at the level of a batch: what shadows its shared decoder keeps, a shadow's
 * content, and the rounding R over a sequence's cache rows; exported by libgten_host.so (host/capi_kvq4.cpp) beside
 * include/gten_host.h.  The device's part is include/gten_hip_kvq4.h (the switch is set there, before the batch's decoder is
 * created); DESIGN.md 3.24.
 */
#ifndef GTEN_HOST_KVQ4_H
#define GTEN_HOST_KVQ4_H

#include "gten_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the shared decoder of the batch (created by the call if it was not yet): bits per quant of its shadows (4, 8, 16; 0: none), the
 * bytes of one chunk of one matrix, the bytes of all shadows.  Any output may be NULL.  0, or -1 */
int gten_host_batch_kv_shadow_info(gten_host_batch* b, int* bits, int* chunk_bytes, unsigned long long* bytes_total);

/* R (csrc/gten_kvq4_math.h) in place on cache rows [0, n_rows) of sequence seq, every layer, K and V: afterwards the rows hold what a
 * 4-bit shadow holds of them.  The writes are announced, so a decoder that shadows the rows re-imports them.  0, or non-zero */
int gten_host_batch_kv_round_q4(gten_host_batch* b, int seq, int n_rows);

/* rows [0, n_rows) of sequence seq's own shadow on `layer` as dense Q8 rows [n_rows][kv row bytes] (gten_host_batch_kv_read's
 * shape): k_out and v_out in host memory, either may be NULL.  Refused where the decoder keeps no 4-bit shadows. */
int gten_host_batch_kv_shadow_read(gten_host_batch* b, int seq, int layer, int n_rows, void* k_out, void* v_out);

/* where sequence seq's cache rows of `layer` lie: the device addresses of K and V row 0 and the rows' pitch in bytes -- a row view
 * for the operators of include/gten_hip.h and gten_hip_kv_round_q4 (writers announce their ranges themselves).  Outputs may be NULL. */
int gten_host_batch_kv_rows(gten_host_batch* b, int seq, int layer, void** k_rows, void** v_rows, size_t* pitch);

#ifdef __cplusplus
}
#endif
#endif
