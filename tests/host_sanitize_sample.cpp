// not gpu: host/capi_sample.cpp's sampled serve on the CPU against tests/hip_stub.cpp + tests/hip_stub_sample.cpp, in a binary
// built with -fsanitize=address,undefined (tests/test_sampler_cpu.py).  With top_k 1 the sampled serve returns the greedy
// serve's ids, and every admitted prompt's request reached the slot that took it (stream = its queue index).  Exits 0 when
// every check holds.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/gten_hip.h"
#include "../include/gten_host_sample.h"

extern "C" int hip_stub_sampling_calls(void);
extern "C" int hip_stub_sampling_call(int i, int* seq, int* top_k, float* temp, uint64_t* seed, uint32_t* stream);

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) { std::fprintf(stderr, "host_sanitize_sample: %s failed (line %d)\n", #c, __LINE__); return 1; } \
    } while (0)

int main()
{
    gten_host_config cfg{};
    cfg.n_vocab = 97; cfg.max_ctx = 96; cfg.n_embd = 256; cfg.n_ffn = 512; cfg.n_layers = 2; cfg.n_heads = 4; cfg.n_kv_heads = 2;
    cfg.wdtype = GTEN_Q4; cfg.adtype = GTEN_Q8;
    const int lengths[] = {5, 40, 1, 17, 60, 9, 33, 2, 64, 12, 7, 21};
    const int NP = (int)(sizeof lengths / sizeof lengths[0]), MP = 64, total = 90;
    std::vector<int32_t> prompts((size_t)NP * MP, 0), n_prompt((size_t)NP);
    for (int j = 0; j < NP; j++) {
        n_prompt[(size_t)j] = lengths[j];
        gten_host_synthetic_tokens(prompts.data() + (size_t)j * MP, lengths[j], 500u + 3u * (unsigned)j, cfg.n_vocab);
    }
    gten_host_batch* b = gten_host_batch_create(&cfg, 2);
    CHECK(b);
    CHECK(gten_host_batch_load_synthetic(b, 99) == 0);
    const int W = total > MP ? total : MP;
    std::vector<int32_t> want((size_t)NP * W), got((size_t)NP * W), nw((size_t)NP), ng((size_t)NP);
    CHECK(gten_host_batch_serve2(b, prompts.data(), n_prompt.data(), NP, MP, total, -1, 8, 0, nullptr, want.data(), nw.data(), nullptr, 0) == 0);
    std::vector<int32_t> ks((size_t)NP, 1);
    std::vector<float> ts((size_t)NP);
    for (int j = 0; j < NP; j++) ts[(size_t)j] = 0.5f + 0.25f * (float)j;
    const int before = hip_stub_sampling_calls();
    double st[9];
    CHECK(gten_host_batch_serve_topk(b, prompts.data(), n_prompt.data(), NP, MP, total, -1, 8, 0, nullptr, got.data(), ng.data(), st, 9,
                                     ks.data(), ts.data(), 0, 0.f, 0xABCDEF0123456789ull) == 0);
    for (int j = 0; j < NP; j++) {
        CHECK(ng[(size_t)j] == nw[(size_t)j]);
        for (int i = 0; i < nw[(size_t)j]; i++) CHECK(got[(size_t)j * W + i] == want[(size_t)j * W + i]);
    }
    // every prompt that reached a slot: a request with its stream, top_k and temp; afterwards every slot greedy again
    std::vector<char> seen((size_t)NP, 0);
    int seq = 0, k = 0;
    float t = 0.f;
    uint64_t seed = 0;
    uint32_t stream = 0;
    const int after = hip_stub_sampling_calls();
    for (int i = before; i < after - 2; i++) {
        CHECK(hip_stub_sampling_call(i, &seq, &k, &t, &seed, &stream) == 0);
        CHECK(stream < (uint32_t)NP && seq >= 0 && seq < 2);
        CHECK(k == 1 && t == ts[stream] && seed == 0xABCDEF0123456789ull);
        seen[stream] = 1;
    }
    for (int i = after - 2; i < after; i++) {
        CHECK(hip_stub_sampling_call(i, &seq, &k, &t, &seed, &stream) == 0);
        CHECK(k == 0);
    }
    for (int j = 0; j < NP; j++) CHECK(seen[(size_t)j] || nw[(size_t)j] <= lengths[j] + 1);
    CHECK(gten_host_batch_serve_topk(b, prompts.data(), n_prompt.data(), NP, MP, total, -1, 8, 0, nullptr, got.data(), ng.data(), st, 9,
                                     ks.data(), nullptr, -1, 0.f, 1) != 0);            // a bad request is refused
    gten_host_batch_free(b);
    std::printf("host_sanitize_sample ok\n");
    return 0;
}
