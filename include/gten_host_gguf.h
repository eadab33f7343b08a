/*
 * gten_host_gguf.h -- a model's weights from the tensors of a GGUF file, as they lie in the file; exported by libgten_host.so
 * (host/capi_gguf.cpp, host/quant_load.h).  The device's part is include/gten_hip_gguf.h, which defines what the six ggml block
 * formats decode to and the row map; DESIGN.md 3.29.  The file itself is read by tinyllama.cpp_amd/convert.py (open_gguf) or
 * host/gguf_file.h; these calls take one tensor's bytes.
 */
#ifndef GTEN_HOST_GGUF_H
#define GTEN_HOST_GGUF_H

#include "gten_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Weight idx (the .gten record order) from the bytes of a GGUF tensor of ggml type ggml_type.  A block format (Q4_0 2, Q5_0 6,
 * Q8_0 8, Q4_K 12, Q5_K 13, Q6_K 14): nbytes must be the block stream's size for the tensor's shape; the bytes go up through the
 * staging buffer of gten_host_quant.h (kept until the release call there) and are decoded, row-mapped by n_head (0: identity;
 * attn_q takes the head count, attn_k the K/V head count) and quantised into the model's weight dtype by one launch.  F32 (0),
 * F16 (1) and BF16 (30), which every norm vector is: routed to the dense call of gten_host_quant.h; they take no row map here
 * (n_head must be 0).  0; -1 bad index or argument; -2 wrong size; -3 a type code that is not one of the nine, a block format
 * for a norm vector, or a dense type with n_head != 0; else the device library's code, its text in the device library's last
 * error -- a decoded NaN or infinity is refused there. */
int gten_host_model_set_weight_from_gguf(gten_host_model* m, int idx, const void* bytes, size_t nbytes, int ggml_type, int n_head);

#ifdef __cplusplus
}
#endif
#endif
