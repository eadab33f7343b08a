// capi_gguf.cpp -- flat C export of include/gten_host_gguf.h: a model's weight from the bytes of a GGUF tensor, decoded and quantised
// on the device (host/quant_load.h).
#include "../../include/gten_host_gguf.h"

#include "capi_handles.h"

using namespace gten;

extern "C" {

int gten_host_model_set_weight_from_gguf(gten_host_model* m, int idx, const void* bytes, size_t nbytes, int ggml_type, int n_head)
{
    if (!m) return -1;
    return m->quant.set_weight_from_gguf(*m->model, idx, bytes, nbytes, ggml_type, n_head);
}

} // extern "C"
