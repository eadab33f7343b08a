// capi_prefixes.cpp -- flat C exports of SEVERAL shared prompt prefixes (include/gten_host_prefixes.h).  Kept apart from capi.cpp
// like capi_prefix.cpp: this is the only translation unit that refers to the device entry points of include/gten_hip_prefixes.h; it
// hands them to host/tinyllama_model.h's hooks (detail::prefixes_decode) when the library is loaded.
#include "../../include/gten_host_prefixes.h"
#include "../../include/gten_hip_prefixes.h"

#include "capi_handles.h"

using namespace gten;

static_assert(kPrefixesMax == GTEN_PREFIXES_MAX, "host/prefix_match.h and include/gten_hip_prefixes.h disagree");

namespace {

const bool installed = [] {
    detail::prefixes_decode().set = gten_hip_decoder_prefixes_set;
    detail::prefixes_decode().share = gten_hip_decoder_prefixes_share;
    detail::prefixes_decode().info = gten_hip_decoder_prefixes_info;
    return true;
}();

bool index_ok(int which) { return which >= 0 && which < kPrefixesMax; }

} // namespace

extern "C" {

int gten_host_batch_prefixes_set(gten_host_batch* b, int which, const int32_t* tokens, int n)
{
    if (!b || !index_ok(which) || n < 0 || (n > 0 && !tokens) || !installed) return -1;
    return b->batch->set_prefix_at(which, tokens, n);
}

int gten_host_batch_prefixes_info(gten_host_batch* b, int which, int* n_prefix, unsigned long long* prompts_shared, unsigned long long* rows_computed)
{
    if (!b || !index_ok(which)) return -1;
    if (n_prefix) *n_prefix = b->batch->prefix_len_at(which);
    if (prompts_shared) *prompts_shared = b->batch->prompts_shared_at(which);
    if (rows_computed) *rows_computed = b->batch->rows_computed_at(which);
    return 0;
}

int gten_host_batch_prefixes_decode_info(gten_host_batch* b, int seq, int* which_out, int* chunks_out, int which, int* n_prefix,
                                         unsigned long long* prefix_imports, int* sharers)
{
    if (!b || seq < 0 || seq >= b->batch->n_seq() || !index_ok(which)) return -1;
    b->batch->prefixes_decode_info(seq, which, which_out, chunks_out, n_prefix, prefix_imports, sharers);
    return 0;
}

int gten_host_batch_prefixes_decode_share(gten_host_batch* b, int seq, int which, int rows)
{
    if (!b || seq < 0 || seq >= b->batch->n_seq() || rows < 0) return -1;
    return b->batch->prefixes_share_rc(seq, which, rows);             // (a bad index is the decoder's refusal)
}

int gten_host_batch_prefixes_steps(gten_host_batch* b, int which, const int32_t* tokens, int count, int n_first, int steps)
{
    if (!b || !index_ok(which) || !tokens || count <= 0 || count > b->cfg.max_ctx || n_first < 1 || steps < 0 || n_first + steps - 1 > count) return -1;
    return b->batch->prefix_set_steps(which, tokens, count, n_first, steps);
}

int gten_host_prefixes_match(const int32_t* prefix_ids, const int* lens, int n_prefixes, int max_len, const int32_t* prompt, int n)
{
    return prefixes_match(prefix_ids, lens, n_prefixes, max_len, prompt, n);
}

} // extern "C"
