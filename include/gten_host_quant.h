/*
 * gten_host_quant.h -- a model's weights from UNQUANTISED elements, quantised on the device; exported by libgten_host.so
 * (host/capi_quant.cpp, host/quant_load.h).  The device's part is include/gten_hip_quant.h, whose source dtype codes
 * (GTEN_HIP_SRC_F32 / _BF16 / _F16) these calls take; DESIGN.md 3.26.  gten_host_model_set_weight and
 * gten_host_model_load_gten (gten_host.h) stay the way for bytes that tinyllama.cpp_amd/convert.py has already quantised:
 * both ways leave the same bytes in the weight tensors.
 */
#ifndef GTEN_HOST_QUANT_H
#define GTEN_HOST_QUANT_H

#include "gten_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Weight idx (the .gten record order of gten_host_model_set_weight) from its dense elements in src_dtype: nbytes must be
 * gten_hip_quant_src_bytes(src_dtype, rows, cols) of the tensor.  The bytes are uploaded into a staging buffer the model grows
 * on demand and keeps until gten_host_model_quant_release, then quantised into the weight tensor in the model's weight dtype;
 * norm vectors (f16 in every mode) go the same way.  0; -1 bad index or dtype; -2 wrong size; else the device library's code
 * with its text in gten_hip_last_error() -- a NaN or an infinity among the elements is refused there. */
int gten_host_model_set_weight_from(gten_host_model* m, int idx, const void* bytes, size_t nbytes, int src_dtype);

/* frees the staging buffer (the next set_weight_from allocates it again) */
int gten_host_model_quant_release(gten_host_model* m);

/* An f16 .gten file into a model of any of the three weight dtypes.  An f16 model: gten_host_model_load_gten.  A Q8 or Q4 model:
 * set_weight_from(..., GTEN_HIP_SRC_F16) per record, each payload checked against the tensor's f16 size with the loader's
 * messages; the staging buffer is released at the end.  -1 when the file cannot be opened. */
int gten_host_model_load_gten_f16(gten_host_model* m, const char* path);

/* The bytes weight idx holds in HBM, as the operators read them (the packed layout of gten_hip.h for Q8 / Q4): nbytes must be
 * gten_host_model_weight_bytes(m, idx).  Waits for the stream.  What the tests compare between the two ways of loading. */
int gten_host_model_weight_read(gten_host_model* m, int idx, void* out, size_t nbytes);

#ifdef __cplusplus
}
#endif
#endif
