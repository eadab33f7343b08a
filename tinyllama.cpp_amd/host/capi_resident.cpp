// capi_resident.cpp -- flat C exports of include/gten_host_resident.h: what a model's or a batch's decoder decided about resident
// weights, and host/resident_plan.h itself for callers without a device.  The one host unit that names include/gten_hip_ab.h.
#include "../../include/gten_host_resident.h"
#include "../../include/gten_host_ab.h"

#include "../../include/gten_hip_ab.h"
#include "../../include/gten_hip_oplanes.h"
#include "capi_handles.h"
#include "resident_plan.h"

using namespace gten;

namespace {

int info(gten_hip_decoder* dec, int* launches, long long* bytes, long long* budget, long long* overhead)
{
    if (!dec) return -1;
    if (gten_hip_decoder_resident(dec, launches, bytes)) return -1;
    if (gten_hip_decoder_resident_budget(dec, budget, overhead)) return -1;
    return 0;
}

} // namespace

extern "C" {

int gten_host_model_resident(gten_host_model* m, int* launches, long long* bytes, long long* budget, long long* overhead)
{
    if (!m) return -1;
    return info(m->model->decoder_handle(), launches, bytes, budget, overhead);
}

int gten_host_batch_resident(gten_host_batch* b, int* launches, long long* bytes, long long* budget, long long* overhead)
{
    if (!b) return -1;
    return info(b->batch->decoder_handle(), launches, bytes, budget, overhead);
}

int gten_host_model_o_planes(gten_host_model* m, int* planes)
{
    if (!m) return -1;
    gten_hip_decoder* dec = m->model->decoder_handle();
    return (dec && !gten_hip_decoder_o_planes(dec, planes)) ? 0 : -1;
}

int gten_host_batch_o_planes(gten_host_batch* b, int* planes)
{
    if (!b) return -1;
    gten_hip_decoder* dec = b->batch->decoder_handle();
    return (dec && !gten_hip_decoder_o_planes(dec, planes)) ? 0 : -1;
}

int gten_host_resident_plan(int n_layers, int n_embd, int n_ffn, int kv_width, int n_vocab, int block_bytes, long long budget,
                            unsigned char* resident_out, long long* launch_bytes_out, long long* bytes_out)
{
    if (n_layers < 0 || n_embd <= 0 || n_ffn <= 0 || kv_width <= 0 || n_vocab <= 0 || block_bytes <= 0 || n_embd % 32 || n_ffn % 32) return -1;
    const std::vector<ResidentLaunch> step = resident_step_launches(n_layers, n_embd, n_ffn, kv_width, n_vocab, block_bytes);
    const ResidentPlan p = resident_plan(step, budget);
    for (size_t i = 0; i < step.size(); i++) {
        if (resident_out) resident_out[i] = (unsigned char)p.resident[i];
        if (launch_bytes_out) launch_bytes_out[i] = step[i].bytes;
    }
    if (bytes_out) *bytes_out = p.bytes;
    return p.launches;
}

} // extern "C"
