// generate.h -- choosing the next id, once for every entry point above the C ABI of libgten_hip.so: greedy, top-k sampling
// (include/gten_hip_sample.h), bias tables (include/gten_hip_bias.h) and log-prob records
// (include/gten_hip_logprobs.h), top-p / min-p cuts (include/gten_hip_nucleus.h) and penalties on
// repeated ids (include/gten_hip_penalty.h) and token automata (include/gten_hip_fsm.h) are ONE flow with optional stages -- a Request says what a prompt asks for, a
// compile-time mask says which device entry points the flow may name.
//
// Why a mask and not a run-time switch: host/capi.cpp links against a stand-in of include/gten_hip.h alone
// (tests/test_host_sanitize_cpu.py), host/capi.cpp + host/capi_sample.cpp against that plus the sampler's
// (tests/test_sampler_cpu.py).  So every flow here is a template on the mask, the stages it does not have are discarded with
// `if constexpr`, and each flow is instantiated where its stages may be named: mask 0 in host/capi.cpp, kSampled in
// host/capi_sample.cpp, kSampled | kBiased in host/capi_bias.cpp, those three in host/capi_logprobs.cpp, four in host/capi_nucleus.cpp, five in host/capi_penalty.cpp, all six in host/capi_fsm.cpp
// (and in the command line program, which links against the library itself).  That is the only reason those files are separate.
#pragma once

#include <cmath>

#include "tinyllama_model.h"
#include "../../include/gten_hip_sample.h"
#include "../../include/gten_hip_bias.h"
#include "../../include/gten_hip_logprobs.h"
#include "../../include/gten_hip_nucleus.h"
#include "../../include/gten_hip_penalty.h"
#include "../../include/gten_hip_fsm.h"
#include "../../include/gten_hip_mirostat.h"

namespace gten {

// (kPenalty -- include/gten_hip_penalty.h, DESIGN.md §3.14, instantiated in host/capi_penalty.cpp -- requires kSampled: a penalised
// greedy request takes its first id from the device too)
// (kFsm -- include/gten_hip_fsm.h, DESIGN.md §3.15, instantiated in host/capi_fsm.cpp -- requires kSampled for the same reason)
// (kMirostat -- include/gten_hip_mirostat.h, DESIGN.md §3.23, instantiated in host/capi_mirostat.cpp and the command line only -- requires
// kSampled: Mirostat acts on a sampling request)
enum : unsigned { kSampled = 1u, kBiased = 2u, kLogprobs = 4u, kNucleus = 8u, kPenalty = 16u, kFsm = 32u, kMirostat = 64u };

// why a prompt's generation ended (kFsm flows report it per item)
enum : int { kEndedByLength = 0, kEndedByEos = 1, kEndedByFinal = 2 };

// What one prompt or sequence asks for.  The defaults: greedy, no table, no records.
struct Request {
    int top_k = 0;               // 0: greedy
    float temp = 0.f;
    uint64_t seed = 0;
    uint32_t stream = 0;         // the draw at a position is keyed by (seed, stream, position)
    int table = -1;              // bias table (-1: none) ...
    int min_new = 0;             // ... which holds for the first min_new new ids (0: for all of them)
    int n_top = -1;              // alternatives per log-prob record (0: the id's own log-prob only; -1: no records)
    float top_p = 1.f, min_p = 0.f;      // the cut of the draw ((1, 0): none; ignored by a greedy request)
    float rep = 1.f, freq = 0.f, pres = 0.f;     // the penalties on ids the sequence already holds ((1, 0, 0): none; they act on greedy too)
    int last_n = 0;                      // ... counted over the last last_n positions (0: all of them) ...
    bool count_prompt = true;            // ... the prompt's included, or only what was generated
    int fsm_start = -1;                  // the state of the decoder's automaton pool the first new id is chosen in (-1: no automaton)
    int shift_keep = -1, shift_drop = 0; // context shift when the window fills (host/generate_shift.h; keep < 0: off, the sequence ends there)
    float miro_tau = 0.f, miro_eta = 0.1f;       // Mirostat v2's target surprise in bits and learning rate (tau 0: off; ignored by a greedy request)
    bool mirostat() const { return top_k > 0 && miro_tau != 0.f; }
    bool cuts() const { return top_k > 0 && !(top_p == 1.f && min_p == 0.f); }
    bool penalises() const { return !(rep == 1.f && freq == 0.f && pres == 0.f); }
    int start(int n_prompt) const { return count_prompt ? 0 : n_prompt; }
    // the first position the table no longer holds at, for a prompt of n_prompt ids (0: it holds throughout)
    int until(int n_prompt) const { return (table >= 0 && min_new > 0) ? n_prompt + min_new : 0; }
};

inline bool request_ok(int top_k, float temp) { return top_k >= 0 && (top_k == 0 || (std::isfinite(temp) && temp > 0.f)); }
inline bool binding_ok(int table, int min_new) { return table >= -1 && table < GTEN_HIP_BIAS_TABLES && min_new >= 0; }
inline bool asking_ok(int n_top, int n_top_max) { return n_top >= -1 && n_top <= GTEN_HIP_LOGPROBS_TOP && n_top <= n_top_max; }
inline bool cut_ok(float top_p, float min_p) { return std::isfinite(top_p) && top_p > 0.f && top_p <= 1.f && std::isfinite(min_p) && min_p >= 0.f && min_p <= 1.f; }
// (tau 0 is "off"; a cut and Mirostat on one request are refused: they do not compose, include/gten_hip_mirostat.h)
inline bool mirostat_ok(float tau, float eta, int top_k, float top_p, float min_p)
{
    if (tau == 0.f) return true;
    if (!(tau > 0.f && tau <= 32.f && eta > 0.f && eta <= 1.f)) return false;
    return !(top_k > 0 && !(top_p == 1.f && min_p == 0.f));
}
inline bool fsm_ok(int fsm_start, int table) { return fsm_start >= -1 && fsm_start < GTEN_HIP_FSM_MAX_STATES && !(fsm_start >= 0 && table >= 0); }
inline bool penalty_ok(float rep, float freq, float pres, int last_n)
{
    return std::isfinite(rep) && rep >= GTEN_HIP_PENALTY_R_MIN && rep <= GTEN_HIP_PENALTY_R_MAX && std::isfinite(freq) &&
           std::fabs(freq) <= GTEN_HIP_PENALTY_ADD_MAX && std::isfinite(pres) && std::fabs(pres) <= GTEN_HIP_PENALTY_ADD_MAX && last_n >= 0;
}

// the requests of a fixed batch's sequences or of a queue's prompts, as the C ABI passes them
struct Requests {
    Each<int32_t> top_k{nullptr, 0};
    Each<float> temp{nullptr, 0.f};
    uint64_t seed = 0;
    const uint32_t* stream = nullptr;        // (null: item j draws with stream j)
    Each<int32_t> table{nullptr, -1}, min_new{nullptr, 0}, n_top{nullptr, -1};
    Each<float> top_p{nullptr, 1.f}, min_p{nullptr, 0.f};
    Each<float> rep{nullptr, 1.f}, freq{nullptr, 0.f}, pres{nullptr, 0.f};
    Each<int32_t> last_n{nullptr, 0}, count_prompt{nullptr, 1};
    Each<int32_t> fsm_start{nullptr, -1};
    Each<float> miro_tau{nullptr, 0.f}, miro_eta{nullptr, 0.1f};
    // these requests under Mirostat (each list may be null: the value for all)
    Requests with_mirostat(const float* tau, float tau_all, const float* eta, float eta_all) const
    {
        Requests r = *this;
        r.miro_tau = {tau, tau_all}; r.miro_eta = {eta, eta_all};
        return r;
    }
    // these requests with a start state per item (null: fsm_all for everybody)
    Requests bound_to(const int32_t* starts, int fsm_all = -1) const
    {
        Requests r = *this;
        r.fsm_start = {starts, fsm_all};
        return r;
    }
    // these requests with a penalty per item (each list may be null: the value for all)
    Requests penalised(const float* rep_, float rep_all, const float* freq_, float freq_all, const float* pres_, float pres_all, const int32_t* last_n_,
                       int last_n_all, const int32_t* count_prompt_, int count_prompt_all) const
    {
        Requests r = *this;
        r.rep = {rep_, rep_all}; r.freq = {freq_, freq_all}; r.pres = {pres_, pres_all};
        r.last_n = {last_n_, last_n_all}; r.count_prompt = {count_prompt_, count_prompt_all};
        return r;
    }
    static Requests of(const int32_t* top_k, int top_k_all, const float* temp, float temp_all, uint64_t seed, const uint32_t* stream = nullptr,
                       const int32_t* table = nullptr, const int32_t* min_new = nullptr, const int32_t* n_top = nullptr,
                       const float* top_p = nullptr, float top_p_all = 1.f, const float* min_p = nullptr, float min_p_all = 0.f)
    {
        Requests r;
        r.top_k = {top_k, top_k_all}; r.temp = {temp, temp_all}; r.seed = seed; r.stream = stream;
        r.table = {table, -1}; r.min_new = {min_new, 0}; r.n_top = {n_top, -1}; r.top_p = {top_p, top_p_all}; r.min_p = {min_p, min_p_all};
        return r;
    }
    Request operator[](int j) const
    {
        Request r{top_k[j], temp[j], seed, stream ? stream[j] : (uint32_t)j, table[j], min_new[j], n_top[j], top_p[j], min_p[j],
                  rep[j], freq[j], pres[j], last_n[j], count_prompt[j] != 0, fsm_start[j]};
        r.miro_tau = miro_tau[j]; r.miro_eta = miro_eta[j];
        return r;
    }
    bool ok(int n, int n_top_max) const
    {
        for (int j = 0; j < n; j++)
            if (!request_ok(top_k[j], temp[j]) || !binding_ok(table[j], min_new[j]) || !asking_ok(n_top[j], n_top_max) || !cut_ok(top_p[j], min_p[j]) ||
                !penalty_ok(rep[j], freq[j], pres[j], last_n[j]) || !fsm_ok(fsm_start[j], table[j]) ||
                !mirostat_ok(miro_tau[j], miro_eta[j], top_k[j], top_p[j], min_p[j])) return false;
        return true;
    }
};

// gten_hip_row_top_logprobs' outputs for one row, behind each other on the device: the record of a prompt's first id
struct FirstRecord {
    float logprob;
    int32_t top_id[GTEN_HIP_LOGPROBS_TOP];
    float top_lp[GTEN_HIP_LOGPROBS_TOP];
};
struct FirstRecords {
    FirstRecord* dev = nullptr;
    int rows = 0;
    FirstRecords() = default;
    FirstRecords(const FirstRecords&) = delete;
    ~FirstRecords() { if (dev) gten_hip_free(dev); }
    void ensure(int n)
    {
        if (n <= rows) return;
        if (dev) GTEN_HIP_OK(gten_hip_free(dev));
        dev = nullptr;
        GTEN_HIP_OK(gten_hip_malloc((void**)&dev, (size_t)n * sizeof(FirstRecord)));
        rows = n;
    }
};

// A caller's record outputs: one entry per position, top_id / top_lp n_top_max wide.  No record: log-probs 0, ids -1.
struct RecordRows {
    float* logprob = nullptr;
    int32_t* top_id = nullptr;
    float* top_lp = nullptr;
    int n_top_max = 0;
    // (a caller none of whose requests asks may pass no outputs at all)
    RecordRows from(size_t pos) const
    {
        if (!logprob) return *this;
        return {logprob + pos, top_id + pos * (size_t)n_top_max, top_lp + pos * (size_t)n_top_max, n_top_max};
    }
    void blank(size_t positions) const
    {
        if (!logprob) return;
        std::fill(logprob, logprob + positions, 0.f);
        if (n_top_max > 0) {
            std::fill(top_id, top_id + positions * (size_t)n_top_max, -1);
            std::fill(top_lp, top_lp + positions * (size_t)n_top_max, 0.f);
        }
    }
    // `count` records of n_top entries each (ids and lps dense) into the positions from `pos` on
    void store(size_t pos, int count, int n_top, const float* lp, const int32_t* ids, const float* lps) const
    {
        std::memcpy(logprob + pos, lp, (size_t)count * sizeof(float));
        for (int i = 0; i < count && n_top > 0; i++) {
            std::memcpy(top_id + (pos + (size_t)i) * (size_t)n_top_max, ids + (size_t)i * n_top, (size_t)n_top * sizeof(int32_t));
            std::memcpy(top_lp + (pos + (size_t)i) * (size_t)n_top_max, lps + (size_t)i * n_top, (size_t)n_top * sizeof(float));
        }
    }
    // a first id's record from the device (the stream has been waited for: the id was read back)
    void store_first(size_t pos, int n_top, const FirstRecord* dev) const
    {
        FirstRecord r;
        GTEN_HIP_OK(gten_hip_memcpy_d2h(&r, dev, sizeof(r)));
        store(pos, 1, n_top, &r.logprob, r.top_id, r.top_lp);
    }
    // the decoder's records of sequence seq at positions [pos, pos + count)
    int store_decoded(gten_hip_decoder* dec, int seq, int pos, int count, int n_top) const
    {
        if (count <= 0) return 0;
        std::vector<int32_t> ids((size_t)count * (size_t)std::max(n_top, 1));
        std::vector<float> lps(ids.size()), lp((size_t)count);
        if (const int rc = gten_hip_decoder_logprobs(dec, seq, pos, count, n_top, lp.data(), ids.data(), lps.data())) return rc;
        store((size_t)pos, count, n_top, lp.data(), ids.data(), lps.data());
        return 0;
    }
};

// What a flow keeps of a decoder's automaton pool on the host (kFsm): the flags, read once -- the pool cannot change while a sequence
// is bound -- and one device word for the next state gten_hip_sample_rows_fsm returns with a first id (`after`: that state, -1 for a
// banned id, which only a row whose allowed logits are all -inf yields).
struct FsmHost {
    gten_hip_decoder* dec = nullptr;
    std::vector<uint8_t> flags;
    int32_t* word = nullptr;             // device
    int32_t after = -1;
    // (kMirostat) what gten_hip_sample_rows_miro returned with a first id: the mu the decoder is bound with at the next position
    gten_hip_miro_info* miro_word = nullptr;     // device
    int32_t mu_next = 0;
    gten_hip_miro_info* miro_info_dev()
    {
        if (!miro_word) GTEN_HIP_OK(gten_hip_malloc((void**)&miro_word, sizeof(gten_hip_miro_info)));
        return miro_word;
    }
    void read_mu_next()
    {
        gten_hip_miro_info info;
        GTEN_HIP_OK(gten_hip_memcpy_d2h(&info, miro_word, sizeof(info)));
        mu_next = info.mu_next;
    }
    explicit FsmHost(gten_hip_decoder* dec_ = nullptr) : dec{dec_} {}
    FsmHost(const FsmHost&) = delete;
    ~FsmHost() { if (word) gten_hip_free(word); if (miro_word) gten_hip_free(miro_word); }
    int32_t* next_state_dev()
    {
        if (!word) GTEN_HIP_OK(gten_hip_malloc((void**)&word, sizeof(int32_t)));
        return word;
    }
    void read_after()
    {
        GTEN_HIP_OK(gten_hip_memcpy_d2h(&after, word, sizeof(after)));
        if (after < 0 || after >= GTEN_HIP_FSM_MAX_STATES) after = -1;
    }
    bool final(int state)
    {
        if (flags.empty()) {
            const uint8_t* dev = nullptr;
            int S = 0;
            GTEN_HIP_OK(gten_hip_decoder_fsm_info(dec, &S, nullptr, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, &dev));
            flags.resize((size_t)std::max(S, 1), 0);
            if (S > 0) GTEN_HIP_OK(gten_hip_memcpy_d2h(flags.data(), dev, (size_t)S));
        }
        return state >= 0 && (size_t)state < flags.size() && (flags[(size_t)state] & GTEN_HIP_FSM_FINAL) != 0;
    }
};

// The id that will sit at position `pos`, drawn on the device from the logits row lg into id_dev: plain or under the request's
// table, plus its record into rec_dev when the request asks.  (The only draw from a prompt's row outside the decoder.)
// A penalising request (kPenalty) draws from the row penalised by the prompt's window of ids[0, pos) -- the window the decoder's
// first step would read from its own copy of them.
// A bound request (kFsm) draws in its start state from the row masked by the decoder's pool (gten_hip_sample_rows_fsm: the penalty
// first, the mask second; no table); fsm->after receives the state the id entered, from the operator itself.
template <unsigned M>
void draw_first(gten_hip_decoder* dec, const Request& r, const float* lg, int n_vocab, int32_t pos, int32_t* id_dev, FirstRecord* rec_dev,
                const int32_t* ids = nullptr, FsmHost* fsm = nullptr)
{
    static_assert(M & kSampled, "greedy takes the argmax of the prompt's logits on the host");
    const int32_t k = r.top_k;
    const float* row = nullptr;
    bool drawn = false;
    if constexpr ((M & kBiased) != 0)
        if (r.table >= 0) GTEN_HIP_OK(gten_hip_decoder_bias_info(dec, nullptr, nullptr, nullptr, r.table, &row));
    // A request under Mirostat (kMirostat) draws through gten_hip_sample_rows_miro with the default start mu = 2 tau -- penalised, then under
    // its table or in its start state, never under a cut; fsm->mu_next receives the mu of the next position, from the operator itself.
    if constexpr ((M & kMirostat) != 0)
        if (r.mirostat() && fsm) {
            const uint16_t* next = nullptr;
            const uint8_t* flags = nullptr;
            int S = 0;
            const bool bound = (M & kFsm) != 0 && r.fsm_start >= 0;
            if (bound) GTEN_HIP_OK(gten_hip_decoder_fsm_info(dec, &S, nullptr, nullptr, nullptr, 0, 0, 0, nullptr, &next, &flags));
            const bool pen = (M & kPenalty) != 0 && r.penalises();
            const int32_t lo = pen ? std::min(std::max(std::max(r.start(pos), r.last_n > 0 ? pos - r.last_n : 0), 0), pos) : pos;
            const int32_t off[2] = {0, pos - lo};
            int32_t tq = 0, eq = 0;
            GTEN_ASSERTM(gten_hip_miro_q16_host(r.miro_tau, r.miro_eta, &tq, &eq) == 0, "mirostat tau %g eta %g", (double)r.miro_tau, (double)r.miro_eta);
            const int32_t mu0 = 2 * tq;
            GTEN_HIP_OK(gten_hip_sample_rows_miro(lg, 1, n_vocab, 0, bound ? nullptr : row, 0, bound ? next : nullptr, bound ? flags : nullptr, bound ? S : 0,
                                                  bound ? &r.fsm_start : nullptr, &k, &r.temp, r.seed, &r.stream, &pos, pen ? ids + lo : nullptr,
                                                  pen ? off : nullptr, &r.rep, &r.freq, &r.pres, &mu0, &r.miro_tau, &r.miro_eta, id_dev,
                                                  bound ? fsm->next_state_dev() : nullptr, fsm->miro_info_dev()));
            if (bound) fsm->read_after();
            fsm->read_mu_next();
            drawn = true;
        }
    if constexpr ((M & kFsm) != 0)
        if (r.fsm_start >= 0 && !drawn) {
            const uint16_t* next = nullptr;
            const uint8_t* flags = nullptr;
            int S = 0;
            GTEN_HIP_OK(gten_hip_decoder_fsm_info(dec, &S, nullptr, nullptr, nullptr, 0, 0, 0, nullptr, &next, &flags));
            const bool pen = (M & kPenalty) != 0 && r.penalises();
            const int32_t lo = pen ? std::min(std::max(std::max(r.start(pos), r.last_n > 0 ? pos - r.last_n : 0), 0), pos) : pos;
            const int32_t off[2] = {0, pos - lo};
            const float top_p = r.cuts() ? r.top_p : 1.f, min_p = r.cuts() ? r.min_p : 0.f;
            GTEN_HIP_OK(gten_hip_sample_rows_fsm(lg, 1, n_vocab, 0, next, flags, S, &r.fsm_start, &k, &r.temp, r.seed, &r.stream, &pos, &top_p, &min_p,
                                                 pen ? ids + lo : nullptr, pen ? off : nullptr, &r.rep, &r.freq, &r.pres, id_dev, fsm ? fsm->next_state_dev() : nullptr, nullptr));
            if (fsm) fsm->read_after();
            drawn = true;
        }
    if constexpr ((M & kPenalty) != 0)
        if (r.penalises() && !drawn) {
            const int32_t lo = std::min(std::max(std::max(r.start(pos), r.last_n > 0 ? pos - r.last_n : 0), 0), pos);
            const int32_t off[2] = {0, pos - lo};
            const float top_p = r.cuts() ? r.top_p : 1.f, min_p = r.cuts() ? r.min_p : 0.f;
            GTEN_HIP_OK(gten_hip_sample_rows_pen(lg, 1, n_vocab, 0, row, 0, &k, &r.temp, r.seed, &r.stream, &pos, &top_p, &min_p, ids + lo, off, &r.rep, &r.freq,
                                                 &r.pres, id_dev, nullptr));
            drawn = true;
        }
    if constexpr ((M & kNucleus) != 0)
        if (r.cuts() && !drawn) {
            GTEN_HIP_OK(gten_hip_sample_rows_cut(lg, 1, n_vocab, 0, row, 0, &k, &r.temp, r.seed, &r.stream, &pos, &r.top_p, &r.min_p, id_dev, nullptr));
            drawn = true;
        }
    if constexpr ((M & kBiased) != 0) {
        if (row && !drawn) GTEN_HIP_OK(gten_hip_sample_rows_biased(lg, 1, n_vocab, 0, row, 0, &k, &r.temp, r.seed, &r.stream, &pos, id_dev));
    }
    if (!row && !drawn) GTEN_HIP_OK(gten_hip_sample_rows(lg, 1, n_vocab, 0, &k, &r.temp, r.seed, &r.stream, &pos, id_dev));
    if constexpr ((M & kLogprobs) != 0)
        if (r.n_top >= 0) GTEN_HIP_OK(gten_hip_row_top_logprobs(lg, 1, n_vocab, n_vocab, id_dev, r.n_top, &rec_dev->logprob, rec_dev->top_id, rec_dev->top_lp));
}

// the state sequence q's id at position `pos` is chosen in, as the steps left it
inline int fsm_state_at(gten_hip_decoder* dec, int q, int pos)
{
    int32_t s = -1;
    GTEN_HIP_OK(gten_hip_decoder_slot_states(dec, q, pos, 1, &s));
    return s;
}

// Requests on a decoder's slots [0, n_slots), taken back when the scope ends: whatever way a flow is left, every kind of request
// it has set is cleared on every slot -- the decoder's later steps are greedy, unbound and record nothing.
template <unsigned M>
struct SlotRequests {
    gten_hip_decoder* dec;
    int n_slots;
    bool bound = false, sampling = false, fsm_bound = false, miro_bound = false;
    SlotRequests(gten_hip_decoder* dec_, int n_slots_) : dec{dec_}, n_slots{n_slots_} {}
    SlotRequests(const SlotRequests&) = delete;
    ~SlotRequests() { clear(); }
    // table and log-prob request of a prompt of n_prompt ids (a decoder that refuses them says so here, before any work)
    int bind(int q, const Request& r, int n_prompt)
    {
        (void)q; (void)r; (void)n_prompt;
        if constexpr ((M & (kBiased | kLogprobs | kNucleus | kPenalty)) != 0) bound = true;
        // (a slot that carried a bound prompt is unbound before a table may be set on it: the two do not compose)
        if constexpr ((M & kFsm) != 0) {
            if (fsm_bound)
                if (const int rc = gten_hip_decoder_set_seq_fsm(dec, q, -1, 0)) return rc;
            // (a start state outside the decoder's pool is refused here, before any work, in the setter's own words)
            if (r.fsm_start >= 0) {
                int S = 0;
                if (const int rc = gten_hip_decoder_fsm_info(dec, &S, nullptr, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, nullptr)) return rc;
                if (r.fsm_start >= S) return gten_hip_decoder_set_seq_fsm(dec, q, r.fsm_start, 1);
            }
        }
        // (a slot that carried a prompt under Mirostat is unbound before a cut may be set on it: the two do not compose)
        if constexpr ((M & kMirostat) != 0)
            if (miro_bound)
                if (const int rc = gten_hip_decoder_set_seq_mirostat(dec, q, 0.f, 0.f, 0, 0)) return rc;
        if constexpr ((M & kBiased) != 0)
            if (const int rc = gten_hip_decoder_set_seq_bias(dec, q, r.table, r.until(n_prompt))) return rc;
        if constexpr ((M & kLogprobs) != 0)
            if (const int rc = gten_hip_decoder_set_logprobs(dec, q, r.n_top)) return rc;
        if constexpr ((M & kNucleus) != 0)
            // (a greedy request's cut could never act: it is not passed on, so it does not switch a decoder to the cut launch)
            if (const int rc = gten_hip_decoder_set_cut(dec, q, r.cuts() ? r.top_p : 1.f, r.cuts() ? r.min_p : 0.f)) return rc;
        if constexpr ((M & kPenalty) != 0) {
            const bool on = r.penalises();
            if (const int rc = gten_hip_decoder_set_penalty(dec, q, on ? r.rep : 1.f, on ? r.freq : 0.f, on ? r.pres : 0.f, on ? r.start(n_prompt) : 0,
                                                            on ? r.last_n : 0)) return rc;
        }
        return 0;
    }
    // "the id at position pos of slot q is chosen in `state`" for the decode steps that follow (state < 0: not bound)
    int fsm(int q, int state, int pos)
    {
        (void)q; (void)state; (void)pos;
        if constexpr ((M & kFsm) != 0) {
            if (state < 0) return fsm_bound ? gten_hip_decoder_set_seq_fsm(dec, q, -1, 0) : 0;
            fsm_bound = true;
            return gten_hip_decoder_set_seq_fsm(dec, q, state, pos);
        }
        return 0;
    }
    // "slot q's ids from position pos on are drawn under the request's Mirostat, from mu" for the decode steps that follow (a request
    // without Mirostat: the slot is unbound)
    int mirostat(int q, const Request& r, int32_t mu, int pos)
    {
        (void)q; (void)r; (void)mu; (void)pos;
        if constexpr ((M & kMirostat) != 0) {
            if (!r.mirostat()) return miro_bound ? gten_hip_decoder_set_seq_mirostat(dec, q, 0.f, 0.f, 0, 0) : 0;
            miro_bound = true;
            return gten_hip_decoder_set_seq_mirostat(dec, q, r.miro_tau, r.miro_eta, mu, pos);
        }
        return 0;
    }
    // the sampling request of the decode steps that follow
    int sample(int q, const Request& r)
    {
        (void)q; (void)r;
        if constexpr ((M & kSampled) != 0) {
            sampling = true;
            return gten_hip_decoder_set_sampling(dec, q, r.top_k, r.temp, r.seed, r.stream);
        }
        return 0;
    }
    // 0, or the code of the last call that failed
    int clear()
    {
        int rc = 0;
        if constexpr ((M & kSampled) != 0)
            for (int q = 0; sampling && q < n_slots; q++)
                if (const int r = gten_hip_decoder_set_sampling(dec, q, 0, 0.f, 0, 0)) rc = r;
        if constexpr ((M & kBiased) != 0)
            for (int q = 0; bound && q < n_slots; q++)
                if (const int r = gten_hip_decoder_set_seq_bias(dec, q, -1, 0)) rc = r;
        if constexpr ((M & kLogprobs) != 0)
            for (int q = 0; bound && q < n_slots; q++)
                if (const int r = gten_hip_decoder_set_logprobs(dec, q, -1)) rc = r;
        if constexpr ((M & kNucleus) != 0)
            for (int q = 0; bound && q < n_slots; q++)
                if (const int r = gten_hip_decoder_set_cut(dec, q, 1.f, 0.f)) rc = r;
        if constexpr ((M & kPenalty) != 0)
            for (int q = 0; bound && q < n_slots; q++)
                if (const int r = gten_hip_decoder_set_penalty(dec, q, 1.f, 0.f, 0.f, 0, 0)) rc = r;
        if constexpr ((M & kFsm) != 0)
            for (int q = 0; fsm_bound && q < n_slots; q++)
                if (const int r = gten_hip_decoder_set_seq_fsm(dec, q, -1, 0)) rc = r;
        if constexpr ((M & kMirostat) != 0)
            for (int q = 0; miro_bound && q < n_slots; q++)
                if (const int r = gten_hip_decoder_set_seq_mirostat(dec, q, 0.f, 0.f, 0, 0)) rc = r;
        bound = sampling = fsm_bound = miro_bound = false;
        return rc;
    }
};

// ---- one sequence.  The prompt is processed as in the reference (iteration 0 of greedy_sample); its first id is the host
// argmax of its logits (mask 0) or draw_first's; every later id comes from back-to-back graph replays whose sampler feeds the
// next step on the device -- no logits copy, no host round trip per token.  Mask 0 gives greedy_sample's ids (tested), top_k 0
// gives mask 0's.  With kLogprobs `rows` (max(n_predict, prompt) positions, blanked here once the decoder has accepted the requests)
// receives the new ids' records at their positions.
// Returns the number of ids in `tokens`; -1 when the decoder refuses a request (gten_hip_last_error).
template <unsigned M>
int generate(TinyLlama& model, std::vector<int32_t>& tokens, const int n_predict, const int eos, const Request& r = {}, const RecordRows& rows = {},
             int* ended_by = nullptr, int max_ctx = 0)
{
    const int n_prompt = (int)tokens.size();
    int ended = kEndedByLength, state = -1;
    struct Report { int* out; const int& v; ~Report() { if (out) *out = v; } } report{ended_by, ended};
    (void)state;
    auto blank = [&]() {
        if constexpr ((M & kLogprobs) != 0) rows.blank((size_t)std::max(n_predict, n_prompt));
    };
    if (n_prompt >= n_predict) { blank(); return n_prompt; }
    gten_hip_decoder* dec = nullptr;
    if constexpr (M != 0) dec = model.decoder_handle();
    SlotRequests<M> slot(dec, 1);
    FsmHost fh(dec);
    if (slot.bind(0, r, n_prompt) != 0) return -1;
    blank();
    {
        Tensor input{tokens.data(), {n_prompt}, kInt32};
        const Tensor logits = model.logits(input, 0);
        int32_t first = 0;
        if constexpr (M == 0) {
            const float* p = logits.data_ptr<float>();
            float best = -std::numeric_limits<float>::infinity();
            for (int j = 0; j < logits.numel(); j++)
                if (p[j] > best) { best = p[j]; first = j; }
        } else {
            Tensor id({1}, kInt32);
            FirstRecords rec;
            if constexpr ((M & kLogprobs) != 0) rec.ensure(1);
            draw_first<M>(dec, r, (const float*)logits.device_ptr(), logits.numel(), n_prompt, (int32_t*)id.device_ptr_mut(), rec.dev, tokens.data(), &fh);
            state = fh.after;
            GTEN_HIP_OK(gten_hip_memcpy_d2h(&first, id.device_ptr(), sizeof(first)));
            if constexpr ((M & kLogprobs) != 0)
                if (first != eos && r.n_top >= 0) rows.store_first((size_t)n_prompt, r.n_top, rec.dev);
        }
        if (first == eos) { ended = kEndedByEos; return n_prompt; }
        tokens.push_back(first);
    }
    const int n_first = n_prompt + 1;
    // (a first id that is itself final: the prompt plus that id)
    if constexpr ((M & kFsm) != 0)
        if (r.fsm_start >= 0 && fh.final(state)) { ended = kEndedByFinal; return n_first; }
    const int max_new = n_predict - n_first;
    if (max_new <= 0) return n_first;
    std::vector<int32_t> out((size_t)max_new);
    if (slot.sample(0, r) != 0) return -1;
    if constexpr ((M & kFsm) != 0)
        if (r.fsm_start >= 0 && slot.fsm(0, state, n_first) != 0) return -1;
    if constexpr ((M & kMirostat) != 0)
        if (slot.mirostat(0, r, fh.mu_next, n_first) != 0) return -1;
    const int got = model.decode_generate(tokens.data(), n_first, max_new, eos, out.data());
    tokens.insert(tokens.end(), out.begin(), out.begin() + got);
    // (fewer ids than the steps that could run: an eos.  The context bounds them too; a caller that does not say how long it is
    //  keeps max_tokens inside it)
    if (got < (max_ctx > 0 ? std::min(max_new, max_ctx - n_first + 1) : max_new)) ended = kEndedByEos;
    if constexpr ((M & kFsm) != 0)
        if (r.fsm_start >= 0 && got > 0 && fh.final(fsm_state_at(dec, 0, n_first + got))) ended = kEndedByFinal;
    if constexpr ((M & kLogprobs) != 0)
        if (r.n_top >= 0 && rows.store_decoded(dec, 0, n_first, got, r.n_top) != 0) return -1;
    return slot.clear() ? -1 : (int)tokens.size();
}

// generate() on a caller's array: `tokens` holds n_prompt ids and has room for max(max_tokens, n_prompt)
template <unsigned M>
int generate_in_place(TinyLlama& model, int32_t* tokens, int n_prompt, int max_tokens, int eos, const Request& r = {}, const RecordRows& rows = {},
                      int* ended_by = nullptr, int max_ctx = 0)
{
    std::vector<int32_t> t(tokens, tokens + n_prompt);
    t.reserve((size_t)std::max(max_tokens, n_prompt));
    const int total = generate<M>(model, t, max_tokens, eos, r, rows, ended_by, max_ctx);
    if (total > 0) std::memcpy(tokens, t.data(), (size_t)total * sizeof(int32_t));
    return total;
}

// the first id of `prompt` processed onto cache set `set` of a batch: TinyLlamaBatch::prefill's argmax (mask 0) or draw_first's
template <unsigned M>
int first_id(TinyLlamaBatch& b, int set, const std::vector<int32_t>& prompt, const Request& r, FirstRecord* rec_dev, FsmHost* fsm = nullptr)
{
    if constexpr (M == 0) {
        (void)r; (void)rec_dev; (void)fsm;
        return b.prefill(set, prompt);
    } else {
        gten_hip_decoder* dec = nullptr;
        if constexpr ((M & (kBiased | kNucleus | kFsm)) != 0) dec = b.decoder_handle();
        return b.prefill_picked(set, prompt, [&](int, const float* lg, int n, int32_t* out) {
            draw_first<M>(dec, r, lg, n, (int32_t)prompt.size(), out, rec_dev, prompt.data(), fsm);
        });
    }
}

// ---- a fixed batch (gten_host_batch_generate and its _topk / _biased / _lp forms).  prompts [n_seq][max_prompt] (sequence q uses
// its first n_prompt[q] ids): every request is set first (a refusal comes before any work), each prompt is processed on its
// sequence's own caches and its first id chosen from its logits row, then all sequences generate together with the sampler on
// the device.  out is [n_seq][max_tokens]: prompt + new ids; n_total [n_seq]; rows (kLogprobs) [n_seq][max_tokens] positions.
// 0; -1: bad arguments (nothing was touched); otherwise the code of the decoder call that refused.
template <unsigned M>
int generate_batch(TinyLlamaBatch& batch, int max_ctx, const int32_t* prompts, const int32_t* n_prompt, int max_prompt, int max_tokens, int eos,
                   const Requests& reqs, int32_t* out, int32_t* n_total, const RecordRows& rows = {}, int32_t* ended_by = nullptr)
{
    const int S = batch.n_seq();
    for (int q = 0; q < S; q++)
        if (n_prompt[q] <= 0 || n_prompt[q] > max_prompt || n_prompt[q] >= max_tokens || n_prompt[q] >= max_ctx) return -1;
    if (!reqs.ok(S, rows.n_top_max)) return -1;
    if constexpr ((M & kLogprobs) != 0) rows.blank((size_t)S * (size_t)max_tokens);
    gten_hip_decoder* dec = nullptr;
    if constexpr (M != 0) dec = batch.decoder_handle();
    SlotRequests<M> slots(dec, S);
    FsmHost fh(dec);
    for (int q = 0; q < S; q++)
        if (const int rc = slots.bind(q, reqs[q], n_prompt[q])) return rc;
    std::vector<int32_t> first((size_t)S), state((size_t)S, -1), mu_first((size_t)S, 0);
    std::vector<char> final_first((size_t)S, 0);                  // (kFsm) the first id entered a final state: the prompt plus that id
    FirstRecords rec;
    if constexpr ((M & kLogprobs) != 0) rec.ensure(1);
    for (int q = 0; q < S; q++) {
        const int P = n_prompt[q];
        int32_t* row = out + (size_t)q * max_tokens;
        std::memcpy(row, prompts + (size_t)q * max_prompt, (size_t)P * sizeof(int32_t));
        const Request r = reqs[q];
        first[(size_t)q] = first_id<M>(batch, q, std::vector<int32_t>(row, row + P), r, rec.dev, &fh);
        if constexpr ((M & kFsm) != 0) {
            state[(size_t)q] = fh.after;
            final_first[(size_t)q] = r.fsm_start >= 0 && first[(size_t)q] != eos && fh.final(state[(size_t)q]);
        }
        if constexpr ((M & kMirostat) != 0) mu_first[(size_t)q] = fh.mu_next;
        if constexpr ((M & kLogprobs) != 0)
            if (r.n_top >= 0 && first[(size_t)q] != eos) rows.from((size_t)q * max_tokens).store_first((size_t)P, r.n_top, rec.dev);
    }
    std::vector<int> n_first((size_t)S), room((size_t)S);
    int max_new = 0;
    for (int q = 0; q < S; q++) {
        const int P = n_prompt[q];
        int32_t* row = out + (size_t)q * max_tokens;
        row[P] = first[(size_t)q];                                 // (an eos here ends the sequence below)
        n_first[(size_t)q] = P + 1;
        batch.decode_set_tokens(q, row, 0, P + 1);
        if (const int rc = slots.sample(q, reqs[q])) return rc;
        if constexpr ((M & kFsm) != 0)
            if (reqs[q].fsm_start >= 0 && first[(size_t)q] != eos && !final_first[(size_t)q])
                if (const int rc = slots.fsm(q, state[(size_t)q], P + 1)) return rc;
        if constexpr ((M & kMirostat) != 0)
            if (const int rc = slots.mirostat(q, reqs[q], mu_first[(size_t)q], P + 1)) return rc;
        // this sequence's own room; none when its first id is already eos (the sequence is then parked from the start instead of
        // being decoded for the longest sequence's length)
        room[(size_t)q] = (first[(size_t)q] == eos || final_first[(size_t)q]) ? 0 : max_tokens - (P + 1);
        max_new = std::max(max_new, room[(size_t)q]);
    }
    std::vector<int32_t> gen((size_t)S * (size_t)std::max(max_new, 1));
    std::vector<int> n_out((size_t)S, 0);
    batch.decode_generate(n_first.data(), max_new, eos, gen.data(), n_out.data(), room.data());
    for (int q = 0; q < S; q++) {
        int32_t* row = out + (size_t)q * max_tokens;
        const int total = n_first[(size_t)q];
        if (ended_by) ended_by[q] = kEndedByLength;
        if (row[total - 1] == eos) { n_total[q] = total - 1; if (ended_by) ended_by[q] = kEndedByEos; continue; }
        if (final_first[(size_t)q]) { n_total[q] = total; if (ended_by) ended_by[q] = kEndedByFinal; continue; }
        const int take = std::min(n_out[(size_t)q], max_tokens - total);
        std::memcpy(row + total, gen.data() + (size_t)q * max_new, (size_t)take * sizeof(int32_t));
        n_total[q] = total + take;
        if (ended_by && take < std::min(room[(size_t)q], max_ctx - total + 1)) ended_by[q] = kEndedByEos;
        if constexpr ((M & kFsm) != 0)
            if (ended_by && reqs[q].fsm_start >= 0 && take > 0 && fh.final(fsm_state_at(dec, q, total + take))) ended_by[q] = kEndedByFinal;
        if constexpr ((M & kLogprobs) != 0)
            if (const int n_top = reqs[q].n_top; n_top >= 0)
                if (const int rc = rows.from((size_t)q * max_tokens).store_decoded(dec, q, total, take, n_top)) return rc;
    }
    return slots.clear();
}

// ---- How TinyLlamaBatch::serve_with picks ids.  Prompt j's request (reqs[j]; stream j) draws its first id from the prompt's
// logits row on the device -- under its table, with its record -- and is set on whichever slot takes the prompt, also when a
// sequence moves in the tail: the ids depend on (seed, j) and the logits only, not on the slot or schedule.  A slot's records
// are read when its prompt ends or moves (collect), before the slot is started again.  Every slot's requests are cleared when
// the queue is done.  Mask 0: the prompt's argmax, the decoder's argmax, nothing set.  `rows` is [prompts][row_len] positions.
template <unsigned M>
struct ServePolicy {
    static constexpr bool kLogprobs = (M & gten::kLogprobs) != 0;
    static constexpr bool kFsm = (M & gten::kFsm) != 0;
    static constexpr bool kMirostat = (M & gten::kMirostat) != 0;
    // (kMirostat) per prompt: the mu its next id is drawn under, as the host last read it
    std::vector<int32_t> miro_mu;
    void note_mu(int j, int32_t mu)
    {
        if (miro_mu.empty()) miro_mu.assign((size_t)std::max(reqs_n, j + 1), 0);
        miro_mu[(size_t)j] = mu;
    }
    // (kMirostat) prompt j goes on in slot q with its next id at position pos: the binding travels with the prompt, at the mu the host read
    void bind_mu(int q, int j, int pos) { GTEN_HIP_OK(slots.mirostat(q, reqs[j], miro_mu.empty() ? 0 : miro_mu[(size_t)j], pos)); }
    // (kMirostat) slot q's next id, at position pos, is prompt j's, and the prompt is about to move to another slot (the tail): its mu is
    // read back to go with it.  A slot that stays keeps its mu row on the device: nothing is read between slices
    void read_mu(int q, int j, int pos)
    {
        if (!reqs[j].mirostat()) return;
        int32_t mu = 0;
        GTEN_HIP_OK(gten_hip_decoder_slot_mus(slots.dec, q, pos, 1, &mu));
        note_mu(j, mu);
    }
    // (kFsm) per prompt: the state its next id is chosen in, as the host last read it (-1: not bound), and whether it entered a final one
    std::vector<int32_t> fsm_state;
    std::vector<char> fsm_ended;
    std::vector<int32_t> fsm_buf;
    FsmHost fh;                          // the pool's flags and the operator's next-state word
    bool final_state(int state) { return fh.final(state); }
    Requests reqs;
    RecordRows rows;
    int row_len;
    SlotRequests<M> slots;
    FirstRecords rec;
    int reqs_n = 0;                      // (kFsm) the number of prompts
    ServePolicy(gten_hip_decoder* dec, int n_slots, const Requests& reqs_, const RecordRows& rows_ = {}, int row_len_ = 0, int n_prompts = 0)
        : reqs{reqs_}, rows{rows_}, row_len{row_len_}, slots(dec, n_slots), reqs_n{n_prompts}
    {
        fh.dec = dec;
        if constexpr (kFsm) { fsm_state.assign((size_t)n_prompts, -1); fsm_ended.assign((size_t)n_prompts, 0); }
    }
    RecordRows rows_of(int j) const { return rows.from((size_t)j * (size_t)row_len); }
    FirstRecord* rec_of(int k) const { return kLogprobs ? rec.dev + k : nullptr; }
    void store_first(int k, int j, int pos)
    {
        if (reqs.n_top[j] >= 0 && pos < row_len) rows_of(j).store_first((size_t)pos, reqs.n_top[j], rec_of(k));
    }
    int first(TinyLlamaBatch& b, int c, const std::vector<int32_t>& row, int j)
    {
        if constexpr (kLogprobs) rec.ensure(1);
        const int id = first_id<M>(b, c, row, reqs[j], rec.dev, &fh);
        if constexpr (kLogprobs) store_first(0, j, (int)row.size());
        if constexpr (kFsm) note_first(j, fh.after);
        if constexpr (kMirostat) note_mu(j, fh.mu_next);
        return id;
    }
    // (kFsm) prompt j's first id entered state `after`
    void note_first(int j, int32_t after)
    {
        if (fsm_state.empty()) { fsm_state.assign((size_t)reqs_n, -1); fsm_ended.assign((size_t)reqs_n, 0); }
        fsm_state[(size_t)j] = reqs.fsm_start[j] >= 0 ? after : -1;
    }
    // (kFsm) whether the id just stored for prompt j -- its first -- entered a final state: the prompt ends there and keeps the id
    bool ended_first(int j)
    {
        if (reqs.fsm_start[j] < 0 || !final_state(fsm_state[(size_t)j])) return false;
        fsm_ended[(size_t)j] = 1;
        return true;
    }
    // (kFsm) prompt j goes on in slot q with its next id at position pos: the binding travels with the prompt, at the state the host read
    void bind_state(int q, int j, int pos) { GTEN_HIP_OK(slots.fsm(q, reqs.fsm_start[j] >= 0 ? fsm_state[(size_t)j] : -1, pos)); }
    // (kFsm) the states that slot q's `count` ids from position `from` on entered (null: prompt j is not bound)
    const int32_t* states(int q, int j, int from, int count)
    {
        if (reqs.fsm_start[j] < 0 || fsm_state[(size_t)j] < 0 || count <= 0) return nullptr;
        fsm_buf.resize((size_t)count);
        GTEN_HIP_OK(gten_hip_decoder_slot_states(slots.dec, q, from + 1, count, fsm_buf.data()));
        fsm_state[(size_t)j] = fsm_buf[(size_t)count - 1];
        return fsm_buf.data();
    }
    bool enters_final(int j, int32_t state)
    {
        if (!final_state(state)) return false;
        fsm_ended[(size_t)j] = 1;
        return true;
    }
    // (copy_of: the items that are copies of another item's prompt pass, TinyLlamaBatch::prefill_many_with; null: none)
    void many(TinyLlamaBatch& b, const std::vector<int>& sets, const std::vector<const std::vector<int32_t>*>& ps, const std::vector<int>& js,
              std::vector<int>* first, const std::vector<int>* copy_of = nullptr, const std::vector<int>* ctx_of = nullptr)
    {
        // (ctx_of, session items: item k keeps rows [0, ctx) of its set and only what follows them in ps[k] goes through the model --
        //  the draw below still speaks of the whole of ps[k]: its position, its ids)
        std::vector<std::vector<int32_t>> tails;
        std::vector<const std::vector<int32_t>*> cps = ps;
        if (ctx_of) {
            tails.resize(ps.size());
            for (size_t k = 0; k < ps.size(); k++)
                if ((*ctx_of)[k] > 0) { tails[k].assign(ps[k]->begin() + (*ctx_of)[k], ps[k]->end()); cps[k] = &tails[k]; }
        }
        if constexpr (M == 0) {
            (void)js;
            b.prefill_many(sets, cps, first, nullptr, copy_of, ctx_of);
        } else {
            if constexpr (kLogprobs) rec.ensure((int)sets.size());
            std::vector<float*> lo((size_t)sets.size(), nullptr);
            b.prefill_many_with(sets, cps, first, &lo, [&](int k, const float* lg, int n, int32_t* out) {
                draw_first<M>(slots.dec, reqs[js[(size_t)k]], lg, n, (int32_t)ps[(size_t)k]->size(), out, rec_of(k), ps[(size_t)k]->data(), &fh);
                if constexpr (kFsm) note_first(js[(size_t)k], fh.after);
                if constexpr (kMirostat) note_mu(js[(size_t)k], fh.mu_next);
            }, copy_of, ctx_of);
            if constexpr (kLogprobs)
                for (size_t k = 0; k < js.size(); k++) store_first((int)k, js[k], (int)ps[k]->size());
        }
    }
    // prompt j (n_prompt ids) starts, or goes on, in slot q
    void apply(int q, int j, int n_prompt)
    {
        const Request r = reqs[j];
        GTEN_HIP_OK(slots.sample(q, r));
        GTEN_HIP_OK(slots.bind(q, r, n_prompt));
    }
    // slot q's records of positions [from, from + count) are prompt j's
    void collect(int q, int j, int from, int count)
    {
        if (reqs.n_top[j] >= 0) GTEN_HIP_OK(rows_of(j).store_decoded(slots.dec, q, from, std::min(count, row_len - from), reqs.n_top[j]));
    }
    void clear() { GTEN_HIP_OK(slots.clear()); }
};

// ---- gten_host_batch_serve2's packing around a queue (and its _topk / _biased / _lp forms): the prompts in, a decoder that
// refuses tables or records heard before the queue starts, the rows and the stats list out.  out and rows are
// (group_of, include/gten_host_samples.h: per item the sample group it belongs to, -1 none; null: no groups)
// max(max_tokens, max_prompt) positions per prompt.  0; -1: bad arguments; otherwise the code of the decoder's refusal.
template <unsigned M>
int serve_queue(TinyLlamaBatch& batch, int max_ctx, const int32_t* prompts, const int32_t* n_prompt, int n_prompts, int max_prompt, int max_tokens,
                int eos, int slice, int max_new, const int32_t* max_new_each, int32_t* out, int32_t* n_total, double* stats, int n_stats,
                const Requests& reqs = {}, const RecordRows& rows = {}, int32_t* ended_by = nullptr, const int32_t* group_of = nullptr,
                const int32_t* session = nullptr)
{
    if (n_prompts <= 0 || max_tokens <= 0 || slice <= 0) return -1;
    const int row_len = std::max(max_tokens, max_prompt);
    // (session, include/gten_host_sessions.h: item j continues session[j] >= 0 -- prompts[j] holds the turn's new ids, possibly
    //  none; the item is the prompt ids(s) + prompts[j], which `out`'s stride and the context must hold)
    std::vector<int> full((size_t)n_prompts);
    {
        std::vector<char> seen((size_t)TinyLlamaBatch::kSessionsMax, 0);
        for (int j = 0; j < n_prompts; j++) {
            const int s = session ? session[j] : -1;
            if (s < -1 || (s >= 0 && (!batch.session_is_open(s) || seen[(size_t)s]))) return -1;
            if (s >= 0) seen[(size_t)s] = 1;
            if (n_prompt[j] < (s >= 0 ? 0 : 1) || n_prompt[j] > max_prompt) return -1;
            full[(size_t)j] = n_prompt[j] + (s >= 0 ? (int)batch.session_ids(s).size() : 0);
            if (full[(size_t)j] < 1 || full[(size_t)j] > max_ctx || full[(size_t)j] > row_len) return -1;
        }
    }
    if (!reqs.ok(n_prompts, rows.n_top_max)) return -1;
    gten_hip_decoder* dec = nullptr;
    if constexpr (M != 0) dec = batch.decoder_handle();
    if constexpr ((M & kLogprobs) != 0) rows.blank((size_t)n_prompts * (size_t)row_len);
    // (slot 0 is as it was at once)
    if constexpr ((M & kBiased) != 0)
        if (reqs.table.each) {
            if (const int rc = gten_hip_decoder_set_seq_bias(dec, 0, 0, 0)) return rc;
            if (const int rc = gten_hip_decoder_set_seq_bias(dec, 0, -1, 0)) return rc;
        }
    if constexpr ((M & kLogprobs) != 0)
        if (reqs.n_top.each) {
            if (const int rc = gten_hip_decoder_set_logprobs(dec, 0, 0)) return rc;
            if (const int rc = gten_hip_decoder_set_logprobs(dec, 0, -1)) return rc;
        }
    if constexpr ((M & kNucleus) != 0)
        for (int j = 0, cutting = 0; j < n_prompts && !cutting; j++)
            if ((cutting = reqs[j].cuts())) {
                if (const int rc = gten_hip_decoder_set_cut(dec, 0, reqs[j].top_p, reqs[j].min_p)) return rc;
                if (const int rc = gten_hip_decoder_set_cut(dec, 0, 1.f, 0.f)) return rc;
            }
    if constexpr ((M & kPenalty) != 0)
        for (int j = 0, pen = 0; j < n_prompts && !pen; j++)
            if ((pen = reqs[j].penalises())) {
                if (const int rc = gten_hip_decoder_set_penalty(dec, 0, reqs[j].rep, reqs[j].freq, reqs[j].pres, 0, reqs[j].last_n)) return rc;
                if (const int rc = gten_hip_decoder_set_penalty(dec, 0, 1.f, 0.f, 0.f, 0, 0)) return rc;
            }
    if constexpr ((M & kFsm) != 0) {
        // (... and every start state is one of the pool's: a refusal comes before the queue starts)
        int S = 0;
        if (const int rc = gten_hip_decoder_fsm_info(dec, &S, nullptr, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, nullptr)) return rc;
        for (int j = 0, bound = 0; j < n_prompts; j++)
            if (const int start = reqs[j].fsm_start; start >= 0 && (!bound || start >= S)) {
                if (const int rc = gten_hip_decoder_set_seq_fsm(dec, 0, start, 1)) return rc;
                if (const int rc = gten_hip_decoder_set_seq_fsm(dec, 0, -1, 0)) return rc;
                bound = 1;
            }
    }
    std::vector<std::vector<int32_t>> ps((size_t)n_prompts), res;
    for (int j = 0; j < n_prompts; j++) {
        if (session && session[j] >= 0) ps[(size_t)j] = batch.session_ids(session[j]);
        ps[(size_t)j].insert(ps[(size_t)j].end(), prompts + (size_t)j * max_prompt, prompts + (size_t)j * max_prompt + n_prompt[j]);
    }
    ServePolicy<M> pick(dec, batch.n_seq(), reqs, rows, row_len, n_prompts);
    const TinyLlamaBatch::ServeStats st = batch.serve_with(ps, max_tokens, eos, slice, &res, {max_new_each, max_new}, {group_of, -1}, pick, {session, -1});
    for (int j = 0; j < n_prompts; j++) {
        const int take = std::min((int)res[(size_t)j].size(), std::max(max_tokens, full[(size_t)j]));
        std::memcpy(out + (size_t)j * row_len, res[(size_t)j].data(), (size_t)take * sizeof(int32_t));
        n_total[j] = take;
        if (ended_by) {
            // (shorter than its own limit: an eos, unless the policy saw a final state)
            const int P = full[(size_t)j];
            const int limit = serve_limit(P, max_tokens, max_ctx, Each<int32_t>{max_new_each, max_new}[j]);
            ended_by[j] = take < limit && P < limit ? kEndedByEos : kEndedByLength;
            if constexpr ((M & kFsm) != 0)
                if (pick.fsm_ended[(size_t)j]) ended_by[j] = kEndedByFinal;
        }
        // (a first id that was the eos is not stored: neither is its record)
        if constexpr ((M & kLogprobs) != 0) rows.from((size_t)j * row_len + (size_t)take).blank((size_t)(row_len - take));
    }
    if (stats) {
        // (exactly n_stats doubles are written: a caller sized for an older, shorter list stays inside its array)
        const double all[] = {(double)st.prompt_tokens, (double)st.new_tokens, (double)st.steps, (double)st.admissions, st.prefill_s, st.decode_s,
                              (double)st.lane_steps, (double)st.lane_rows, (double)st.moved};
        const int have = (int)(sizeof(all) / sizeof(all[0]));
        for (int i = 0; i < n_stats; i++) stats[i] = i < have ? all[i] : 0.0;
    }
    return 0;
}

} // namespace gten
