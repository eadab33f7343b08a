// hip_stub_sample.cpp -- test-only stand-in for the symbols of include/gten_hip_sample.h, beside tests/hip_stub.cpp (host
// memory).  sample_rows is the contract restated on the CPU (tests/sample_ref.py); set_sampling records what it receives.
#include <cmath>
#include <cstdint>
#include <vector>

#include "../include/gten_hip_sample.h"

struct StubSampling { const void* dec; int seq, top_k; float temp; uint64_t seed; uint32_t stream; };
static std::vector<StubSampling> g_calls;

extern "C" int hip_stub_sampling_calls(void) { return (int)g_calls.size(); }
extern "C" int hip_stub_sampling_call(int i, int* seq, int* top_k, float* temp, uint64_t* seed, uint32_t* stream)
{
    if (i < 0 || i >= (int)g_calls.size()) return -1;
    const StubSampling& c = g_calls[(size_t)i];
    *seq = c.seq; *top_k = c.top_k; *temp = c.temp; *seed = c.seed; *stream = c.stream;
    return 0;
}

extern "C" int gten_hip_decoder_set_sampling(gten_hip_decoder* dec, int seq, int top_k, float temp, uint64_t seed, uint32_t stream)
{
    if (!dec || seq < 0 || top_k < 0 || (top_k > 0 && !(std::isfinite(temp) && temp > 0.f))) return -4;
    g_calls.push_back(StubSampling{dec, seq, top_k, temp, seed, stream});
    return 0;
}

static uint32_t philox0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t k0, uint32_t k1)
{
    uint32_t c3 = 0;
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}

extern "C" int gten_hip_sample_rows(const float* logits, int n_rows, int n_vocab, long long row_stride, const int32_t* top_k_host,
                                    const float* temp_host, uint64_t seed, const uint32_t* stream_host, const int32_t* position_host,
                                    int32_t* out)
{
    if (n_rows < 0 || n_vocab < 1 || n_vocab > 65535 || row_stride < 0) return -4;
    for (int r = 0; r < n_rows; r++) {
        const float* x = logits + (size_t)r * (size_t)row_stride;
        const int k = top_k_host[r];
        if (k < 0 || (k > 0 && !(std::isfinite(temp_host[r]) && temp_host[r] > 0.f))) return -4;
        int best = 0;
        for (int j = 1; j < n_vocab; j++)
            if (x[j] > x[best]) best = j;
        if (k == 0) { out[r] = best; continue; }
        // candidates: rank of j = #(larger) + #(equal with a lower index) < k
        double top = -INFINITY;
        int id = 0;
        for (int j = 0; j < n_vocab; j++) {
            int rank = 0;
            for (int i = 0; i < n_vocab && rank < k; i++) rank += (x[i] > x[j]) || (x[i] == x[j] && i < j);
            if (rank >= k) continue;
            const uint32_t w = philox0((uint32_t)j, (uint32_t)position_host[r], stream_host[r], (uint32_t)seed, (uint32_t)(seed >> 32));
            const float u = std::fmin(((float)(w >> 8) + 0.5f) * 0x1p-24f, 0x1.fffffep-1f);
            const double s = ((double)x[j] - (double)x[best]) / (double)temp_host[r] - std::log(-std::log((double)u));
            if (s > top) { top = s; id = j; }
        }
        out[r] = id;
    }
    return 0;
}
