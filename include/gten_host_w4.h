/*
 * gten_host_w4.h -- a model's linear weights from the tensors of a GPTQ or AWQ 4-bit checkpoint, as they lie in the file; exported
 * by libgten_host.so (host/capi_w4.cpp, host/quant_load.h).  The device's part is include/gten_hip_w4.h, which defines the two
 * layouts and what they dequantise to; DESIGN.md 3.30.  The file itself is read by tinyllama.cpp_amd/convert.py (open_quantized).
 */
#ifndef GTEN_HOST_W4_H
#define GTEN_HOST_W4_H

#include "gten_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Weight idx (the .gten record order) from the qweight / qzeros / scales (and g_idx, or NULL) of its linear layer in `layout`
 * (GTEN_W4_GPTQ 0, GTEN_W4_AWQ 1).  Each pointer holds gten_hip_w4_src_bytes(layout, which, rows, cols, group_size) bytes for the
 * tensor's own shape; the four pieces go up, each from a 16-byte boundary, through the staging buffer of gten_host_quant.h (kept
 * until the release call there) and are unpacked, transposed, dequantised and quantised into the model's weight dtype by one
 * launch.  NULL g_idx: g(k) = k / group_size; pass NULL when the file's g_idx is that.  Only q, k, v, o, gate, up, down of a block
 * take it: the other weights are dense in these checkpoints and go gten_host_model_set_weight_from's way.  0; -1 bad index or
 * argument; -2 a shape or group_size the layout cannot hold; -3 embed_tokens, lm_head or a norm vector; else the device library's
 * code, its text in the device library's last error -- an infinite scale and a g_idx entry outside the groups are refused there. */
int gten_host_model_set_weight_from_w4(gten_host_model* m, int idx, const void* qweight, const void* qzeros, const void* scales,
                                       const void* g_idx_or_null, int layout, int zero_offset, int group_size);

#ifdef __cplusplus
}
#endif
#endif
