// capi_lora.cpp -- flat C exports of include/gten_host_lora.h: a model's linear weights from unquantised elements with a LoRA
// adapter merged in on the device (host/quant_load.h).  The one translation unit that reaches gten_hip_quantize_weight_lora.
#include "../../include/gten_host_lora.h"

#include "capi_handles.h"

using namespace gten;

extern "C" {

int gten_host_model_set_weight_from_lora(gten_host_model* m, int idx, const void* bytes, size_t nbytes, int src_dtype,
                                         const void* a, const void* b, int rank, int ab_dtype, float scale)
{
    if (!m) return -1;
    return m->quant.set_weight_from_lora(*m->model, idx, bytes, nbytes, src_dtype, a, b, rank, ab_dtype, scale);
}

const char* gten_host_lora_error(gten_host_model* m)
{
    return m ? m->quant.lora_error() : "";
}

} // extern "C"
