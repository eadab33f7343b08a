// capi_regex.cpp -- flat C exports of include/gten_host_regex.h: regular expressions as ranges of an automaton pool (host/regex_build.h,
// host/fsm_build.h) and the vocabulary's byte strings.  No device call is made here: a pool with such ranges reaches the decoder through
// gten_host_model_set_fsm / gten_host_batch_set_fsm (host/capi_fsm.cpp), which hand the byte automata to the device's expansion.
#include "../../include/gten_host_regex.h"

#include <cstring>
#include <string>
#include <vector>

#include "capi_handles.h"

using namespace gten;

extern "C" {

int gten_host_fsm_set_vocab(gten_host_fsm* f, const uint8_t* bytes, const int32_t* offsets) { return f ? f->pool.set_vocab(bytes, offsets) : -1; }

long long gten_host_tokenizer_vocab_bytes(gten_host_tokenizer* t, int n_vocab, const int32_t* empty_ids, int n_empty, uint8_t* bytes_out, long long cap,
                                          int32_t* offsets_out)
{
    if (!t || n_vocab < 1 || !offsets_out || n_empty < 0 || (n_empty > 0 && !empty_ids) || cap < 0 || (cap > 0 && !bytes_out)) return -1;
    static const int32_t kControl[] = {0, 1, 2};
    if (!empty_ids) { empty_ids = kControl; n_empty = 3; }
    std::vector<char> empty((size_t)n_vocab, 0);
    for (int k = 0; k < n_empty; k++)
        if (empty_ids[k] >= 0 && empty_ids[k] < n_vocab) empty[(size_t)empty_ids[k]] = 1;
    std::string all;
    offsets_out[0] = 0;
    for (int i = 0; i < n_vocab; i++) {
        if (!empty[(size_t)i] && i < t->tok.vocab_size()) all += t->tok.piece_bytes(i);
        if (all.size() > 0x7FFFFFFFull) return -1;
        offsets_out[i + 1] = (int32_t)all.size();
    }
    if ((long long)all.size() <= cap && !all.empty()) std::memcpy(bytes_out, all.data(), all.size());
    return (long long)all.size();
}

int gten_host_fsm_add_regex(gten_host_fsm* f, const char* pattern, int eos, int* error_offset)
{
    if (error_offset) *error_offset = -1;
    if (!f || !pattern) return -1;
    return f->pool.add_regex(pattern, std::strlen(pattern), eos, error_offset);
}

int gten_host_regex_byte_dfa(const char* pattern, uint16_t* next256_out, uint8_t* accept_out, int cap_states, int* error_offset)
{
    if (error_offset) *error_offset = -1;
    if (!pattern || cap_states < 0 || (cap_states > 0 && (!next256_out || !accept_out))) return -1;
    ByteDfa d;
    if (const int rc = regex_compile(pattern, std::strlen(pattern), d, error_offset)) return rc;
    if (d.n_states() <= cap_states) {
        std::memcpy(next256_out, d.next.data(), d.next.size() * sizeof(uint16_t));
        std::memcpy(accept_out, d.accept.data(), d.accept.size());
    }
    return d.n_states();
}

int gten_host_fsm_n_regex(const gten_host_fsm* f)
{
    if (!f) return -1;
    int n = 0;
    for (const FsmPool::Part& p : f->pool.parts()) n += (p.regex >= 0 && f->pool.regex(p.regex).mode == FsmPool::kMatch) ? 1 : 0;
    return n;
}

} // extern "C"
