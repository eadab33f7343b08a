// capi_calib.cpp -- flat C exports of include/gten_host_calib.h: the importance of the block linears' input columns collected
// from prompt passes, and a linear weight quantised through the device's delta search (host/calib.h, host/quant_load.h).  The one
// translation unit that reaches gten_hip_calib_col_energy and gten_hip_quantize_weight_search.
#include "../../include/gten_host_calib.h"

#include "capi_handles.h"

using namespace gten;

namespace {

// the hook of gten/modules.h: the four tensors that feed the block's linears hold the rows the forward has just computed
void collect_rows(void* owner, const AttentionBlock& b, int start_pos)
{
    Calib& c = *static_cast<Calib*>(owner);
    const int layer = Calib::layer_of(*c.model, b, c.n_layers);
    if (layer < 0 || c.rc) return;                            // another model's block; or a collection that has failed already
    const Tensor* in[4] = {&b.attn_norm.acv, &b.attn.qkv_acv, &b.ffn_norm.acv, &b.ffn_gate_proj.acv};
    const int n = in[0]->dimsize(0) - start_pos;
    for (int which = 0; which < 4 && !c.rc; which++) {
        const Tensor& x = *in[which];
        const size_t pitch = (size_t)x.bstride(0);
        if (x.dimsize(0) - start_pos != n || x.dimsize(1) != c.width(which)) { c.rc = -1; return; }
        c.rc = gten_hip_calib_col_energy((const uint8_t*)x.device_ptr() + (size_t)start_pos * pitch, dtype_code(x.dtype()), n, x.dimsize(1),
                                         (long long)pitch, c.at(layer, which));
    }
    if (layer == 0 && !c.rc) c.rows += n;
}

} // namespace

extern "C" {

int gten_host_calib_begin(gten_host_model* m)
{
    if (!m) return -1;
    detail::CalibRows& hook = detail::calib_rows();
    if (hook.call && hook.owner != &m->calib) return -1;
    detail::ensure_runtime();
    if (const int rc = m->calib.reset(m->cfg.n_layers, m->cfg.n_embd, m->cfg.n_ffn)) return rc;
    m->calib.model = m->model.get();
    m->calib.collecting = true;
    hook.call = collect_rows;
    hook.owner = &m->calib;
    return 0;
}

int gten_host_calib_end(gten_host_model* m)
{
    if (!m || !m->calib.collecting) return -1;
    m->calib.stop();
    return m->calib.rc;
}

long long gten_host_calib_rows(gten_host_model* m)
{
    return m ? m->calib.rows : -1;
}

int gten_host_calib_read(gten_host_model* m, int layer, int which, double* out, int n)
{
    if (!m || !out || m->calib.rows < 0 || layer < 0 || layer >= m->calib.n_layers || which < 0 || which > 3) return -1;
    if (n != m->calib.width(which)) return -2;
    return gten_hip_memcpy_d2h(out, m->calib.at(layer, which), (size_t)n * sizeof(double));
}

int gten_host_calib_set_weight_from(gten_host_model* m, int idx, const void* bytes, size_t nbytes, int src_dtype, const float* importance, int n)
{
    if (!m || idx < 0 || idx >= m->model->n_weights()) return -1;
    const int last = m->model->n_weights() - 1;
    const Tensor& w = m->model->weight(idx);
    std::string& said = m->calib.error;
    const std::string head = "calib_set_weight_from: weight " + std::to_string(idx);
    if (idx == 0 || idx >= last - 1 || (idx - 1) % 9 >= 7) {
        said = head + " is " + (idx == 0 ? "embed_tokens" : idx == last ? "lm_head" : "a norm vector") +
               ": only q, k, v, o, gate, up and down of a block are searched";
        return -3;
    }
    if (w.dtype() != kQint4) {
        said = head + ": the model is not q4 (the search writes Q4 blocks only)";
        return -3;
    }
    if (n != w.dimsize(1)) {
        said = head + ": importance of " + std::to_string(n) + " values for " + std::to_string(w.dimsize(1)) + " columns";
        return -3;
    }
    return m->quant.set_weight_from_search(*m->model, idx, bytes, nbytes, src_dtype, importance);
}

const char* gten_host_calib_error(gten_host_model* m)
{
    return m ? m->calib.error.c_str() : "";
}

} // extern "C"
