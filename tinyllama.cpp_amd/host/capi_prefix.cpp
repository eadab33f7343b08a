// capi_prefix.cpp -- flat C exports of the shared prompt prefix (include/gten_host_prefix.h, include/gten_host_prefix_decode.h).
// Kept apart from capi.cpp: this is the only translation unit that refers to the prefixed device entry points
// (include/gten_hip_prefix.h, include/gten_hip_prefix_decode.h); it hands them to the headers' hooks (gten/modules.h,
// detail::prefixed_rows; host/tinyllama_model.h, detail::prefix_decode) when the library is loaded.
#include "../../include/gten_host_prefix.h"
#include "../../include/gten_host_prefix_decode.h"
#include "../../include/gten_hip_prefix.h"
#include "../../include/gten_hip_prefix_decode.h"

#include "capi_handles.h"

using namespace gten;

namespace {

const bool installed = [] {
    detail::prefixed_rows().call = gten_hip_block_rows_prefixed;
    detail::prefix_decode().prefix_set = gten_hip_decoder_prefix_set;
    detail::prefix_decode().slot_share = gten_hip_decoder_slot_share;
    detail::prefix_decode().info = gten_hip_decoder_prefix_info;
    return true;
}();

} // namespace

extern "C" {

int gten_host_batch_set_prefix(gten_host_batch* b, const int32_t* tokens, int n)
{
    if (!b || n < 0 || (n > 0 && !tokens) || !installed) return -1;
    return b->batch->set_prefix(tokens, n);
}

int gten_host_batch_prefix_info(gten_host_batch* b, int* n_prefix, unsigned long long* prompts_shared, unsigned long long* rows_computed)
{
    if (!b) return -1;
    if (n_prefix) *n_prefix = b->batch->prefix_len();
    if (prompts_shared) *prompts_shared = b->batch->prompts_shared();
    if (rows_computed) *rows_computed = b->batch->rows_computed();
    return 0;
}

int gten_host_batch_prefix_decode_info(gten_host_batch* b, int seq, int* n_prefix, int* seq_chunks, unsigned long long* prefix_imports,
                                       unsigned long long* imports_skipping)
{
    if (!b || seq < 0 || seq >= b->batch->n_seq()) return -1;
    b->batch->prefix_decode_info(seq, n_prefix, seq_chunks, prefix_imports, imports_skipping);
    return 0;
}

int gten_host_batch_prefix_decode_share(gten_host_batch* b, int seq, int rows)
{
    if (!b || seq < 0 || seq >= b->batch->n_seq() || rows < 0) return -1;
    return b->batch->slot_share_rc(seq, rows);
}

int gten_host_set_prefix_decode_shared(int on) { return gten_hip_set_prefix_decode_shared(on); }

} // extern "C"
