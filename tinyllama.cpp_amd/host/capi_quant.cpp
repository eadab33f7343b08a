// capi_quant.cpp -- flat C exports of include/gten_host_quant.h: a model's weights from unquantised elements, quantised on the
// device (host/quant_load.h).
#include "../../include/gten_host_quant.h"

#include "capi_handles.h"

using namespace gten;

extern "C" {

int gten_host_model_set_weight_from(gten_host_model* m, int idx, const void* bytes, size_t nbytes, int src_dtype)
{
    if (!m) return -1;
    return m->quant.set_weight_from(*m->model, idx, bytes, nbytes, src_dtype);
}

int gten_host_model_quant_release(gten_host_model* m)
{
    if (!m) return -1;
    m->quant.release();
    return 0;
}

int gten_host_model_load_gten_f16(gten_host_model* m, const char* path)
{
    if (!m || !path) return -1;
    std::ifstream f(path, std::ios::binary);
    if (!f) return -1;
    m->quant.load_gten_f16(*m->model, f);
    return 0;
}

int gten_host_model_weight_read(gten_host_model* m, int idx, void* out, size_t nbytes)
{
    if (!m || !out || idx < 0 || idx >= m->model->n_weights()) return -1;
    Tensor& w = m->model->weight(idx);
    if (nbytes != w.nbytes()) return -2;
    return gten_hip_memcpy_d2h(out, w.device_weight(), nbytes);
}

} // extern "C"
