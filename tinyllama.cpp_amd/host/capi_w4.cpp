// capi_w4.cpp -- flat C export of include/gten_host_w4.h: a model's linear weight from the tensors of a GPTQ / AWQ 4-bit checkpoint,
// unpacked, transposed and quantised on the device (host/quant_load.h).
#include "../../include/gten_host_w4.h"

#include "capi_handles.h"

using namespace gten;

extern "C" {

int gten_host_model_set_weight_from_w4(gten_host_model* m, int idx, const void* qweight, const void* qzeros, const void* scales,
                                       const void* g_idx_or_null, int layout, int zero_offset, int group_size)
{
    if (!m) return -1;
    return m->quant.set_weight_from_w4(*m->model, idx, qweight, qzeros, scales, g_idx_or_null, layout, zero_offset, group_size);
}

} // extern "C"
