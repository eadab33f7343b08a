// capi_logprobs.cpp -- flat C exports of include/gten_host_logprobs.h: generation that reports every new id's log-prob and top-N
// alternatives.  Kept apart from capi.cpp, capi_sample.cpp and capi_bias.cpp: this is the only translation unit that instantiates code
// referring to include/gten_hip_logprobs.h's entry points.
#include "../../include/gten_host_logprobs.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "capi_handles.h"

using namespace gten;

namespace {

bool request_ok(int top_k, float temp)
{
    return top_k >= 0 && (top_k == 0 || (std::isfinite(temp) && temp > 0.f));
}
bool binding_ok(int table, int min_new)
{
    return table >= -1 && table < GTEN_HIP_BIAS_TABLES && min_new >= 0;
}
bool asking_ok(int n_top, int n_top_max)
{
    return n_top >= -1 && n_top <= GTEN_HIP_LOGPROBS_TOP && n_top <= n_top_max;
}

// every position: no record
void blank(float* logprob, int32_t* top_id, float* top_lp, size_t positions, int n_top_max)
{
    std::fill(logprob, logprob + positions, 0.f);
    if (n_top_max > 0) {
        std::fill(top_id, top_id + positions * (size_t)n_top_max, -1);
        std::fill(top_lp, top_lp + positions * (size_t)n_top_max, 0.f);
    }
}

// a first id's record on the device: gten_hip_row_top_logprobs' three outputs behind each other
struct FirstRecord {
    void* dev = nullptr;
    FirstRecord() { GTEN_HIP_OK(gten_hip_malloc(&dev, bytes())); }
    FirstRecord(const FirstRecord&) = delete;
    ~FirstRecord() { if (dev) gten_hip_free(dev); }
    static size_t bytes() { return sizeof(float) + (size_t)GTEN_HIP_LOGPROBS_TOP * (sizeof(int32_t) + sizeof(float)); }
    void compute(const float* lg, int n_vocab, const int32_t* id_dev, int n_top)
    {
        uint8_t* r = (uint8_t*)dev;
        GTEN_HIP_OK(gten_hip_row_top_logprobs(lg, 1, n_vocab, n_vocab, id_dev, n_top, (float*)r, (int32_t*)(r + 4), (float*)(r + 4 + 4 * GTEN_HIP_LOGPROBS_TOP)));
    }
    void store(int n_top, float* logprob, int32_t* top_id, float* top_lp)
    {
        std::vector<uint8_t> h(bytes());
        GTEN_HIP_OK(gten_hip_memcpy_d2h(h.data(), dev, h.size()));
        std::memcpy(logprob, h.data(), sizeof(float));
        if (n_top > 0) {
            std::memcpy(top_id, h.data() + 4, (size_t)n_top * sizeof(int32_t));
            std::memcpy(top_lp, h.data() + 4 + 4 * GTEN_HIP_LOGPROBS_TOP, (size_t)n_top * sizeof(float));
        }
    }
};

// the decoder's records of positions [from, from + count) into rows of n_top_max entries
int read_records(gten_hip_decoder* dec, int seq, int from, int count, int n_top, int n_top_max, float* logprob, int32_t* top_id, float* top_lp)
{
    if (count <= 0) return 0;
    std::vector<int32_t> ids((size_t)count * (size_t)std::max(n_top, 1));
    std::vector<float> lps((size_t)count * (size_t)std::max(n_top, 1));
    if (const int rc = gten_hip_decoder_logprobs(dec, seq, from, count, n_top, logprob + from, ids.data(), lps.data())) return rc;
    for (int i = 0; i < count && n_top > 0; i++) {
        std::memcpy(top_id + (size_t)(from + i) * n_top_max, ids.data() + (size_t)i * n_top, (size_t)n_top * sizeof(int32_t));
        std::memcpy(top_lp + (size_t)(from + i) * n_top_max, lps.data() + (size_t)i * n_top, (size_t)n_top * sizeof(float));
    }
    return 0;
}

} // namespace

extern "C" {

int gten_host_model_set_logprobs(gten_host_model* m, int n_top)
{
    if (!m) return -1;
    return gten_hip_decoder_set_logprobs(m->model->decoder_handle(), 0, n_top);
}

int gten_host_batch_set_logprobs(gten_host_batch* b, int seq, int n_top)
{
    if (!b) return -1;
    return gten_hip_decoder_set_logprobs(b->batch->decoder_handle(), seq, n_top);
}

int gten_host_model_logprobs(gten_host_model* m, int n_from, int count, int n_top, float* logprob_out, int32_t* top_id_out, float* top_logprob_out)
{
    if (!m) return -1;
    return gten_hip_decoder_logprobs(m->model->decoder_handle(), 0, n_from, count, n_top, logprob_out, top_id_out, top_logprob_out);
}

int gten_host_batch_logprobs(gten_host_batch* b, int seq, int n_from, int count, int n_top, float* logprob_out, int32_t* top_id_out,
                             float* top_logprob_out)
{
    if (!b) return -1;
    return gten_hip_decoder_logprobs(b->batch->decoder_handle(), seq, n_from, count, n_top, logprob_out, top_id_out, top_logprob_out);
}

int gten_host_model_generate_lp(gten_host_model* m, int32_t* tokens, int n_prompt, int max_tokens, int eos, int top_k, float temp, uint64_t seed,
                                uint32_t stream, int table, int min_new, int n_top, float* logprob_out, int32_t* top_id_out, float* top_logprob_out)
{
    if (!m || !tokens || n_prompt <= 0 || max_tokens <= 0 || !request_ok(top_k, temp) || !binding_ok(table, min_new)) return -1;
    if (n_top < 0 || n_top > GTEN_HIP_LOGPROBS_TOP || !logprob_out || (n_top > 0 && (!top_id_out || !top_logprob_out))) return -1;
    std::vector<int32_t> t(tokens, tokens + n_prompt), ti;
    std::vector<float> lp, tl;
    t.reserve((size_t)std::max(max_tokens, n_prompt));
    const int total = logprobs_generate(*m->model, t, max_tokens, eos, top_k, temp, seed, stream, table, min_new, n_top, &lp, &ti, &tl);
    if (total < 0) return total;
    blank(logprob_out, top_id_out, top_logprob_out, (size_t)std::max(max_tokens, n_prompt), n_top);
    std::memcpy(tokens, t.data(), (size_t)total * sizeof(int32_t));
    std::memcpy(logprob_out, lp.data(), (size_t)total * sizeof(float));
    if (n_top > 0) {
        std::memcpy(top_id_out, ti.data(), (size_t)total * (size_t)n_top * sizeof(int32_t));
        std::memcpy(top_logprob_out, tl.data(), (size_t)total * (size_t)n_top * sizeof(float));
    }
    return total;
}

// gten_host_batch_generate_biased's flow with a log-prob request per sequence
int gten_host_batch_generate_lp(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int max_prompt, int max_tokens, int eos,
                                const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed, const uint32_t* stream,
                                const int32_t* table, const int32_t* min_new, int32_t* out, int32_t* n_total, const int32_t* n_top, int n_top_max,
                                float* logprob_out, int32_t* top_id_out, float* top_logprob_out)
{
    if (!b || !prompts || !n_prompt || !out || !n_total || max_tokens <= 0) return -1;
    if (n_top_max < 0 || n_top_max > GTEN_HIP_LOGPROBS_TOP || !logprob_out || (n_top_max > 0 && (!top_id_out || !top_logprob_out))) return -1;
    TinyLlamaBatch& batch = *b->batch;
    const int S = batch.n_seq();
    auto k_of = [&](int q) { return top_k ? top_k[q] : top_k_all; };
    auto t_of = [&](int q) { return temp ? temp[q] : temp_all; };
    auto tab_of = [&](int q) { return table ? table[q] : -1; };
    auto top_of = [&](int q) { return n_top ? n_top[q] : -1; };
    auto until_of = [&](int q) { return (tab_of(q) >= 0 && min_new && min_new[q] > 0) ? n_prompt[q] + min_new[q] : 0; };
    for (int q = 0; q < S; q++) {
        const int P = n_prompt[q];
        if (P <= 0 || P > max_prompt || P >= max_tokens || P >= b->cfg.max_ctx) return -1;
        if (!request_ok(k_of(q), t_of(q)) || !binding_ok(tab_of(q), min_new ? min_new[q] : 0) || !asking_ok(top_of(q), n_top_max)) return -1;
    }
    blank(logprob_out, top_id_out, top_logprob_out, (size_t)S * (size_t)max_tokens, n_top_max);
    gten_hip_decoder* dec = batch.decoder_handle();
    auto reset = [&]() {
        int rc = 0;
        for (int q = 0; q < S; q++) {
            if (const int r = batch.decode_set_sampling(q, 0, 0.f, 0, 0)) rc = r;
            if (const int r = gten_hip_decoder_set_seq_bias(dec, q, -1, 0)) rc = r;
            if (const int r = gten_hip_decoder_set_logprobs(dec, q, -1)) rc = r;
        }
        return rc;
    };
    // the bindings and requests first: a refusal (a persistent decoder) before any work
    for (int q = 0; q < S; q++) {
        if (const int rc = gten_hip_decoder_set_seq_bias(dec, q, tab_of(q), until_of(q))) { reset(); return rc; }
        if (const int rc = gten_hip_decoder_set_logprobs(dec, q, top_of(q))) { reset(); return rc; }
    }
    // every prompt on its own caches, its first id drawn from its logits row on the device under its table -- and its record from that row
    std::vector<int32_t> first((size_t)S);
    std::vector<uint32_t> streams((size_t)S);
    FirstRecord fr;
    for (int q = 0; q < S; q++) {
        const int P = n_prompt[q];
        int32_t* row = out + (size_t)q * max_tokens;
        std::memcpy(row, prompts + (size_t)q * max_prompt, (size_t)P * sizeof(int32_t));
        streams[(size_t)q] = stream ? stream[q] : (uint32_t)q;
        const int32_t kk = k_of(q), pos = P;
        const float t = t_of(q);
        const float* brow = nullptr;
        if (tab_of(q) >= 0 && gten_hip_decoder_bias_info(dec, nullptr, nullptr, nullptr, tab_of(q), &brow) != 0) { reset(); return -1; }
        first[(size_t)q] = batch.prefill_picked(q, std::vector<int32_t>(row, row + P), [&](int, const float* lg, int n, int32_t* id) {
            if (brow) GTEN_HIP_OK(gten_hip_sample_rows_biased(lg, 1, n, 0, brow, 0, &kk, &t, seed, &streams[(size_t)q], &pos, id));
            else GTEN_HIP_OK(gten_hip_sample_rows(lg, 1, n, 0, &kk, &t, seed, &streams[(size_t)q], &pos, id));
            if (top_of(q) >= 0) fr.compute(lg, n, id, top_of(q));
        });
        if (top_of(q) >= 0 && first[(size_t)q] != eos) {
            const size_t at = (size_t)q * max_tokens + (size_t)P;
            fr.store(top_of(q), logprob_out + at, top_id_out + at * n_top_max, top_logprob_out + at * n_top_max);
        }
    }
    std::vector<int> n_first((size_t)S), room((size_t)S);
    int max_new = 0;
    for (int q = 0; q < S; q++) {
        const int P = n_prompt[q];
        int32_t* row = out + (size_t)q * max_tokens;
        row[P] = first[(size_t)q];                                 // (an eos here ends the sequence below)
        n_first[(size_t)q] = P + 1;
        batch.decode_set_tokens(q, row, 0, P + 1);
        if (const int rc = batch.decode_set_sampling(q, k_of(q), t_of(q), seed, streams[(size_t)q])) { reset(); return rc; }
        room[(size_t)q] = (first[(size_t)q] == eos) ? 0 : max_tokens - (P + 1);
        max_new = std::max(max_new, room[(size_t)q]);
    }
    std::vector<int32_t> gen((size_t)S * (size_t)std::max(max_new, 1));
    std::vector<int> n_out((size_t)S, 0);
    batch.decode_generate(n_first.data(), max_new, eos, gen.data(), n_out.data(), room.data());
    for (int q = 0; q < S; q++) {
        int32_t* row = out + (size_t)q * max_tokens;
        const int total = n_first[(size_t)q];
        if (row[total - 1] == eos) { n_total[q] = total - 1; continue; }
        const int take = std::min(n_out[(size_t)q], max_tokens - total);
        std::memcpy(row + total, gen.data() + (size_t)q * max_new, (size_t)take * sizeof(int32_t));
        n_total[q] = total + take;
        if (top_of(q) >= 0) {
            const size_t at = (size_t)q * max_tokens;
            if (const int rc = read_records(dec, q, total, take, top_of(q), n_top_max, logprob_out + at, top_id_out + at * n_top_max,
                                            top_logprob_out + at * n_top_max)) { reset(); return rc; }
        }
    }
    return reset();
}

int gten_host_batch_serve_lp(gten_host_batch* b, const int32_t* prompts, const int32_t* n_prompt, int n_prompts, int max_prompt, int max_tokens,
                             int eos, int slice, int max_new, const int32_t* max_new_each, int32_t* out, int32_t* n_total, double* stats, int n_stats,
                             const int32_t* top_k, const float* temp, int top_k_all, float temp_all, uint64_t seed, const int32_t* table,
                             const int32_t* min_new, const int32_t* n_top, int n_top_max, float* logprob_out, int32_t* top_id_out,
                             float* top_logprob_out)
{
    if (!b || !prompts || !n_prompt || !out || !n_total || n_prompts <= 0 || max_prompt <= 0 || n_stats < 0 || (n_stats > 0 && !stats)) return -1;
    if (max_tokens <= 0 || slice <= 0) return -1;
    if (n_top_max < 0 || n_top_max > GTEN_HIP_LOGPROBS_TOP || !logprob_out || (n_top_max > 0 && (!top_id_out || !top_logprob_out))) return -1;
    for (int j = 0; j < n_prompts; j++) {
        if (!request_ok(top_k ? top_k[j] : top_k_all, temp ? temp[j] : temp_all)) return -1;
        if (!binding_ok(table ? table[j] : -1, min_new ? min_new[j] : 0) || !asking_ok(n_top ? n_top[j] : -1, n_top_max)) return -1;
        if (n_prompt[j] <= 0 || n_prompt[j] > max_prompt || n_prompt[j] > b->cfg.max_ctx) return -1;
    }
    const int row_len = std::max(max_tokens, max_prompt);
    blank(logprob_out, top_id_out, top_logprob_out, (size_t)n_prompts * (size_t)row_len, n_top_max);
    gten_hip_decoder* dec = b->batch->decoder_handle();
    // a decoder that refuses tables or requests says so before the queue starts (slot 0 is as it was at once)
    if (table) {
        if (const int rc = gten_hip_decoder_set_seq_bias(dec, 0, 0, 0)) return rc;
        if (const int rc = gten_hip_decoder_set_seq_bias(dec, 0, -1, 0)) return rc;
    }
    if (n_top) {
        if (const int rc = gten_hip_decoder_set_logprobs(dec, 0, 0)) return rc;
        if (const int rc = gten_hip_decoder_set_logprobs(dec, 0, -1)) return rc;
    }
    const TinyLlamaBatch::BiasedServe base{top_k, temp, top_k_all, temp_all, seed, table, min_new, dec};
    TinyLlamaBatch::LpServe pick(base, n_top, n_top_max, row_len, logprob_out, top_id_out, top_logprob_out);
    std::vector<std::vector<int32_t>> ps((size_t)n_prompts), res;
    for (int j = 0; j < n_prompts; j++)
        ps[(size_t)j].assign(prompts + (size_t)j * max_prompt, prompts + (size_t)j * max_prompt + n_prompt[j]);
    const TinyLlamaBatch::ServeStats st = b->batch->serve_with(ps, max_tokens, eos, slice, &res, max_new, max_new_each, pick);
    for (int j = 0; j < n_prompts; j++) {
        const int take = std::min((int)res[(size_t)j].size(), std::max(max_tokens, n_prompt[j]));
        std::memcpy(out + (size_t)j * row_len, res[(size_t)j].data(), (size_t)take * sizeof(int32_t));
        n_total[j] = take;
        // (a first id that was the eos is not stored: neither is its record)
        const size_t at = (size_t)j * row_len + (size_t)take;
        blank(logprob_out + at, top_id_out + at * n_top_max, top_logprob_out + at * n_top_max, (size_t)(row_len - take), n_top_max);
    }
    const double all[] = {(double)st.prompt_tokens, (double)st.new_tokens, (double)st.steps, (double)st.admissions, st.prefill_s, st.decode_s,
                          (double)st.lane_steps, (double)st.lane_rows, (double)st.moved};
    const int have = (int)(sizeof(all) / sizeof(all[0]));
    for (int i = 0; i < n_stats; i++) stats[i] = i < have ? all[i] : 0.0;
    return 0;
}

int gten_host_model_score_top(gten_host_model* m, const int32_t* tokens, int n, int start_pos, const int32_t* targets, int n_top,
                              float* logprob_out, int32_t* rank_out, int32_t* top_id_out, float* top_logprob_out)
{
    if (!m || !tokens || n < 1 || n > m->cfg.max_ctx || start_pos < 0 || start_pos >= n || !targets || !logprob_out) return -1;
    if (n_top < 0 || n_top > GTEN_HIP_LOGPROBS_TOP || (n_top > 0 && (!top_id_out || !top_logprob_out))) return -1;
    const int rows = n - start_pos, V = m->cfg.n_vocab;
    for (int i = 0; i < rows; i++)
        if (targets[i] < -1 || targets[i] >= V) return -1;
    // targets | log-probs | ranks | the operator's log-probs (unused: the scorer's are returned) | top ids | top log-probs
    void* io = nullptr;
    const size_t R = (size_t)rows, T = (size_t)std::max(n_top, 1);
    GTEN_HIP_OK(gten_hip_malloc(&io, R * 4 * (4 + 2 * T)));
    int32_t* tdev = (int32_t*)io;
    float* lp = (float*)(tdev + R);
    int32_t* rk = (int32_t*)(lp + R);
    float* lp2 = (float*)(rk + R);
    int32_t* tid = (int32_t*)(lp2 + R);
    float* tlp = (float*)(tid + R * T);
    GTEN_HIP_OK(gten_hip_memcpy_h2d(tdev, targets, R * sizeof(int32_t)));
    Tensor tk(tokens, {n}, kInt32);
    m->model->rows_logits(tk, start_pos, [&](const float* lg, int r0, int cr, long long stride) {
        GTEN_HIP_OK(gten_hip_row_logprobs(lg, cr, V, stride, tdev + r0, lp + r0, rk + r0, nullptr));
        GTEN_HIP_OK(gten_hip_row_top_logprobs(lg, cr, V, stride, tdev + r0, n_top, lp2 + r0, tid + (size_t)r0 * n_top, tlp + (size_t)r0 * n_top));
    });
    GTEN_HIP_OK(gten_hip_memcpy_d2h(logprob_out, lp, R * sizeof(float)));
    if (rank_out) GTEN_HIP_OK(gten_hip_memcpy_d2h(rank_out, rk, R * sizeof(int32_t)));
    if (n_top > 0) {
        GTEN_HIP_OK(gten_hip_memcpy_d2h(top_id_out, tid, R * (size_t)n_top * sizeof(int32_t)));
        GTEN_HIP_OK(gten_hip_memcpy_d2h(top_logprob_out, tlp, R * (size_t)n_top * sizeof(float)));
    }
    GTEN_HIP_OK(gten_hip_free(io));
    return 0;
}

} // extern "C"
