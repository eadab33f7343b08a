// capi_kvfp8.cpp -- flat C exports of include/gten_host_kvfp8.h: the rounding R over a sequence's f16 cache rows and the read-back of an
// FP8 shadow of a batch's shared decoder.  The one host unit that names include/gten_hip_kvfp8.h.
#include "../../include/gten_host_kvfp8.h"

#include "../../include/gten_hip_kvfp8.h"
#include "capi_handles.h"

using namespace gten;

extern "C" {

int gten_host_batch_kv_round_fp8(gten_host_batch* b, int seq, int n_rows)
{
    if (!b || seq < 0 || seq >= b->batch->n_seq() || n_rows < 1 || n_rows > b->cfg.max_ctx || b->cfg.adtype != GTEN_F16) return -1;
    const size_t rb = gten_hip_row_bytes(b->cfg.adtype, b->cfg.n_embd / b->cfg.n_heads * b->cfg.n_kv_heads);
    for (int l = 0; l < b->cfg.n_layers; l++) {
        AttentionBlock& blk = b->batch->seq(seq).block(l);
        for (auto* acv : {&blk.attn.key.acv, &blk.attn.value.acv})
            if (const int rc = gten_hip_kv_round_fp8(acv->device_ptr_mut(), n_rows, rb, (size_t)acv->bstride(0))) return rc;
    }
    return 0;
}

int gten_host_batch_kv_shadow_read_fp8(gten_host_batch* b, int seq, int layer, int n_rows, void* k_out, void* v_out)
{
    if (!b) return -1;
    gten_hip_decoder* dec = b->batch->decoder_handle();
    if (!dec) return -1;
    void* outs[2] = {k_out, v_out};
    for (int kv = 0; kv < 2; kv++)
        if (outs[kv])
            if (const int rc = gten_hip_decoder_kv_shadow_read_fp8(dec, seq, layer, kv, n_rows, outs[kv])) return rc;
    return 0;
}

} // extern "C"
