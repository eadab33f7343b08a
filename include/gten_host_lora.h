/*
 * gten_host_lora.h -- a model's linear weights from UNQUANTISED elements with a LoRA adapter merged in on the device; exported
 * by libgten_host.so (host/capi_lora.cpp, host/quant_load.h).  The device's part is include/gten_hip_lora.h, which defines the
 * merge (W + scale * B . A, rounded to the source dtype, then quantised as gten_host_quant.h's loader would); DESIGN.md 3.27.
 * One adapter per call, merged for good: loading another adapter is a reload from the same base elements.
 */
#ifndef GTEN_HOST_LORA_H
#define GTEN_HOST_LORA_H

#include "gten_host_quant.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Weight idx (the .gten record order) from its dense elements in src_dtype, as in gten_host_quant.h's loader (nbytes is checked
 * the same way), plus an adapter: a = lora_A [rank][cols], b = lora_B [rows][rank], dense host arrays in ab_dtype (a source
 * dtype code), scale = lora_alpha / r.  A and B are uploaded into a buffer of their own beside the staging buffer; both stay
 * until gten_host_model_quant_release.  Only q, k, v, o, gate, up and down of a block take an adapter.
 * 0; -1 bad index, dtype, rank (1..64) or pointer; -2 wrong size; -3 embed_tokens, lm_head or a norm vector
 * (gten_host_lora_error() names it); else the device library's code with its text in gten_hip_last_error(): a NaN or an infinity
 * in the merged matrix is refused there. */
int gten_host_model_set_weight_from_lora(gten_host_model* m, int idx, const void* bytes, size_t nbytes, int src_dtype,
                                         const void* a, const void* b, int rank, int ab_dtype, float scale);

/* the text of the model's last -3 */
const char* gten_host_lora_error(gten_host_model* m);

#ifdef __cplusplus
}
#endif
#endif
