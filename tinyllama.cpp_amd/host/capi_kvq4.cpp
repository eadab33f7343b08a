// capi_kvq4.cpp -- flat C exports of include/gten_host_kvq4.h: the shadows of a batch's shared decoder and the rounding R over a
// sequence's cache rows.  The one host unit that names include/gten_hip_kvq4.h (host/capi.cpp and the headers it instantiates go on
// linking against the stand-in of include/gten_hip.h alone).
#include "../../include/gten_host_kvq4.h"

#include "../../include/gten_hip_kvq4.h"
#include "capi_handles.h"

using namespace gten;

extern "C" {

int gten_host_batch_kv_shadow_info(gten_host_batch* b, int* bits, int* chunk_bytes, unsigned long long* bytes_total)
{
    if (!b) return -1;
    gten_hip_decoder* dec = b->batch->decoder_handle();
    return (dec && !gten_hip_decoder_kv_shadow_info(dec, bits, chunk_bytes, bytes_total)) ? 0 : -1;
}

int gten_host_batch_kv_round_q4(gten_host_batch* b, int seq, int n_rows)
{
    if (!b || seq < 0 || seq >= b->batch->n_seq() || n_rows < 1 || n_rows > b->cfg.max_ctx || b->cfg.adtype != GTEN_Q8) return -1;
    const size_t rb = gten_hip_row_bytes(b->cfg.adtype, b->cfg.n_embd / b->cfg.n_heads * b->cfg.n_kv_heads);
    for (int l = 0; l < b->cfg.n_layers; l++) {
        AttentionBlock& blk = b->batch->seq(seq).block(l);
        for (auto* acv : {&blk.attn.key.acv, &blk.attn.value.acv})
            if (const int rc = gten_hip_kv_round_q4(acv->device_ptr_mut(), n_rows, rb, (size_t)acv->bstride(0))) return rc;
    }
    return 0;
}

int gten_host_batch_kv_rows(gten_host_batch* b, int seq, int layer, void** k_rows, void** v_rows, size_t* pitch)
{
    if (!b || seq < 0 || seq >= b->batch->n_seq() || layer < 0 || layer >= b->cfg.n_layers) return -1;
    AttentionBlock& blk = b->batch->seq(seq).block(layer);
    if (k_rows) *k_rows = blk.attn.key.acv.device_ptr_mut();
    if (v_rows) *v_rows = blk.attn.value.acv.device_ptr_mut();
    if (pitch) *pitch = (size_t)blk.attn.key.acv.bstride(0);
    return 0;
}

int gten_host_batch_kv_shadow_read(gten_host_batch* b, int seq, int layer, int n_rows, void* k_out, void* v_out)
{
    if (!b) return -1;
    gten_hip_decoder* dec = b->batch->decoder_handle();
    if (!dec) return -1;
    void* outs[2] = {k_out, v_out};
    for (int kv = 0; kv < 2; kv++)
        if (outs[kv])
            if (const int rc = gten_hip_decoder_kv_shadow_read(dec, seq, layer, kv, n_rows, outs[kv])) return rc;
    return 0;
}

} // extern "C"
