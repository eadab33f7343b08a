// capi_generate.cpp -- host/capi_flows.h's three functions: the one instantiation of host/generate.h's flows at kFull in the library.
// Every generation export above kSampled (host/capi_bias.cpp ... host/capi_mirostat.cpp, host/capi_sessions.cpp, host/capi_samples.cpp,
// and host/capi_shift.cpp when no shift is asked for) ends here.
#include "capi_flows.h"

namespace gten {

int generate_full(TinyLlama& model, int32_t* tokens, int n_prompt, int max_tokens, int eos, const Request& r, const RecordRows& rows, int* ended_by, int max_ctx)
{
    return generate_in_place<kFull>(model, tokens, n_prompt, max_tokens, eos, r, rows, ended_by, max_ctx);
}

int generate_batch_full(TinyLlamaBatch& batch, int max_ctx, const int32_t* prompts, const int32_t* n_prompt, int max_prompt, int max_tokens, int eos,
                        const Requests& reqs, int32_t* out, int32_t* n_total, const RecordRows& rows, int32_t* ended_by)
{
    return generate_batch<kFull>(batch, max_ctx, prompts, n_prompt, max_prompt, max_tokens, eos, reqs, out, n_total, rows, ended_by);
}

int serve_queue_full(TinyLlamaBatch& batch, int max_ctx, const int32_t* prompts, const int32_t* n_prompt, int n_prompts, int max_prompt, int max_tokens,
                     int eos, int slice, int max_new, const int32_t* max_new_each, int32_t* out, int32_t* n_total, double* stats, int n_stats,
                     const Requests& reqs, const RecordRows& rows, int32_t* ended_by, const int32_t* group_of, const int32_t* session)
{
    return serve_queue<kFull>(batch, max_ctx, prompts, n_prompt, n_prompts, max_prompt, max_tokens, eos, slice, max_new, max_new_each, out, n_total, stats,
                              n_stats, reqs, rows, ended_by, group_of, session);
}

} // namespace gten
