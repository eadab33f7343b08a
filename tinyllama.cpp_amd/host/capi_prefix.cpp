// capi_prefix.cpp -- flat C exports of the shared prompt prefix (include/gten_host_prefix.h).  Kept apart from capi.cpp: this
// is the only translation unit that refers to the prefixed device entry point (include/gten_hip_prefix.h); it hands it to
// the headers' hook (gten/modules.h, detail::prefixed_rows) when the library is loaded.
#include "../../include/gten_host_prefix.h"
#include "../../include/gten_hip_prefix.h"

#include "capi_handles.h"

using namespace gten;

namespace {

const bool installed = [] {
    detail::prefixed_rows().call = gten_hip_block_rows_prefixed;
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

} // extern "C"
