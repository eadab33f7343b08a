// capi_text.cpp -- flat C exports of include/gten_host_stoptext.h and include/gten_host_json.h: stop strings given as text as search
// ranges of an automaton pool (host/stop_text_build.h, host/fsm_build.h), and JSON schemas as patterns (host/json_schema.h).  No
// device call is made here: a pool with a search range reaches the decoder through gten_host_model_set_fsm / gten_host_batch_set_fsm
// (host/capi_fsm.cpp), which hand the byte automaton to the device's expansion.
#include "../../include/gten_host_stoptext.h"
#include "../../include/gten_host_json.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "capi_handles.h"
#include "json_schema.h"

using namespace gten;

namespace {

// the C interface's (pointer, length) pairs as StopText; false on a null pointer or a negative length
bool strings_of(const uint8_t* const* ptrs, const int32_t* lens, int n, std::vector<StopText>& out)
{
    if (!ptrs || !lens || n < 1) return false;
    for (int k = 0; k < n; k++) {
        if (!ptrs[k] || lens[k] < 0) return false;
        out.push_back(StopText{ptrs[k], (size_t)lens[k]});
    }
    return true;
}

} // namespace

extern "C" {

int gten_host_fsm_add_stop_text(gten_host_fsm* f, const uint8_t* const* ptrs, const int32_t* lens, int n)
{
    std::vector<StopText> s;
    if (!f || !strings_of(ptrs, lens, n, s)) return -1;
    return f->pool.add_stop_text(s.data(), n);
}

int gten_host_fsm_n_search(const gten_host_fsm* f)
{
    if (!f) return -1;
    int n = 0;
    for (const FsmPool::Part& p : f->pool.parts()) n += (p.regex >= 0 && f->pool.regex(p.regex).mode == FsmPool::kSearch) ? 1 : 0;
    return n;
}

int gten_host_stop_text_dfa(const uint8_t* const* ptrs, const int32_t* lens, int n, uint16_t* next256_out, uint8_t* accept_out, int cap_states)
{
    std::vector<StopText> s;
    if (!strings_of(ptrs, lens, n, s) || cap_states < 0 || (cap_states > 0 && (!next256_out || !accept_out))) return -1;
    ByteDfa d;
    if (const int rc = stop_text_build(s.data(), n, d)) return rc;
    if (d.n_states() <= cap_states) {
        std::memcpy(next256_out, d.next.data(), d.next.size() * sizeof(uint16_t));
        std::memcpy(accept_out, d.accept.data(), d.accept.size());
    }
    return d.n_states();
}

int gten_host_stop_text_find(const uint8_t* const* ptrs, const int32_t* lens, int n, const uint8_t* text, long long n_text, long long* begin, long long* end)
{
    std::vector<StopText> s;
    if (!strings_of(ptrs, lens, n, s) || n_text < 0 || (n_text > 0 && !text) || !begin || !end) return -2;
    for (const StopText& t : s)
        if (t.n == 0) return -2;
    const uint8_t none = 0;
    const StopTextHit h = stop_text_find(s.data(), n, text ? text : &none, n_text);
    *begin = h.begin;
    *end = h.end;
    return h.index;
}

long long gten_host_json_schema_regex(const char* schema_text, int ws, int depth, char* out, long long cap, char* error_out, long long error_cap)
{
    if (error_out && error_cap > 0) error_out[0] = 0;
    if (cap < 0 || (cap > 0 && !out)) return -1;
    std::string pattern, error;
    const int rc = json_schema_regex(schema_text, schema_text ? std::strlen(schema_text) : 0, ws, depth, pattern, error);
    if (rc) {
        if (error_out && error_cap > 0) {
            const size_t m = std::min(error.size(), (size_t)error_cap - 1);
            std::memcpy(error_out, error.data(), m);
            error_out[m] = 0;
        }
        return rc;
    }
    if ((long long)pattern.size() < cap) std::memcpy(out, pattern.c_str(), pattern.size() + 1);
    return (long long)pattern.size();
}

} // extern "C"
