/*
 * gten_host_resident.h -- which W.x launches of a decoder keep their weights in the memory-side cache: what a model's or a batch's
 * decoder decided, and the plan itself without a device; exported by libgten_host.so (host/capi_resident.cpp) beside
 * include/gten_host.h.  The device's part is include/gten_hip_ab.h (gten_hip_set_weight_resident_mb); DESIGN.md §3.2.
 */
#ifndef GTEN_HOST_RESIDENT_H
#define GTEN_HOST_RESIDENT_H

#include "gten_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the decoder of a model / of a batch (created by the call if it was not yet): its resident launches and their weight bytes, the bytes
 * it had left for them and what it took off the setting first (gten_hip_decoder_resident, gten_hip_decoder_resident_budget).  Any
 * output may be NULL.  0, or -1 */
int gten_host_model_resident(gten_host_model* m, int* launches, long long* bytes, long long* budget, long long* overhead);
int gten_host_batch_resident(gten_host_batch* b, int* launches, long long* bytes, long long* budget, long long* overhead);

/* ---- the plan (host/resident_plan.h), callable without a device */
/* The W.x launches of one step in step order -- per layer q|k|v, o, gate|up, down, then lm_head: 4 * n_layers + 1 -- of a model whose
 * weight blocks (32 elements, deltas included) take block_bytes, against `budget` bytes.  resident_out[4 * n_layers + 1] (may be
 * NULL): 1 where the launch is resident; launch_bytes_out likewise: every launch's weight bytes.  Returns the number of resident
 * launches, their byte sum in *bytes_out; -1: bad arguments. */
int gten_host_resident_plan(int n_layers, int n_embd, int n_ffn, int kv_width, int n_vocab, int block_bytes, long long budget,
                            unsigned char* resident_out, long long* launch_bytes_out, long long* bytes_out);

#ifdef __cplusplus
}
#endif
#endif
