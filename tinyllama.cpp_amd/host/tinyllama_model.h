// tinyllama_model.h -- the caller of the hot path: model wiring, .gten loader
// and greedy loop, written against the HBM-backed gten API.  Counterpart of the
// reference's tinyllama.cpp:12-76 (params, TinyLlama), 301-392 (loader) and
// 395-440 (greedy sampler).  Generation with the sampler on the device -- greedy,
// top-k, bias tables, log-prob records -- is host/generate.h.
#pragma once

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <fcntl.h>
#include <omp.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <memory>
#include <string>
#include <vector>
#include <deque>

#include "../gten/gten.h"
#include "../../include/gten_hip_score.h"
#include "session_plan.h"
#include "synth.h"
#include "prefix_match.h"

namespace gten {

// tinyllama.cpp:12-20, but runtime-configurable (small parity models)
struct TinyLLamaParams {
    int n_vocab = 32003;
    int max_ctx = 2048;
    int n_embd = 2048;
    int n_ffn = 5632;
    int n_layers = 22;
    int n_heads = 32;
    int n_query_groups = 4;
};

class TinyLlama {
public:
    const TinyLLamaParams params;
    ModuleDtype dtype_;
    int n_ctx_;

public:
    // tinyllama.cpp:30-43
    TinyLlama(const int n_ctx, ModuleDtype dtype, TinyLLamaParams p = TinyLLamaParams{})
        : params{p},
          dtype_{dtype},
          n_ctx_{n_ctx},
          tok_emb_{Embedding(p.n_vocab, p.n_embd, n_ctx, dtype)},
          norm_{RMSNorm(p.n_embd, n_ctx, {kFloat16, dtype.adtype})},
          lm_head_{EmbeddingLinear{p.n_embd, p.n_vocab, n_ctx, {dtype.wdtype, kFloat32}}}
    {
        blocks_.reserve(p.n_layers);
        for (int i = 0; i < p.n_layers; i++)
            blocks_.push_back(AttentionBlock(p.n_heads, p.n_embd, p.n_query_groups, p.n_ffn, n_ctx, dtype));
    }

    // tinyllama.cpp:45-61: the whole token history comes in, rows
    // [start_pos, n) are computed, the result is the f32 logits of the last row.
    Tensor logits(const Tensor& tokens, const int start_pos = 0)
    {
        if (tokens.numel() > n_ctx_) {
            std::cerr << "Number of prompt tokens (" << tokens.numel() << ") exceed provided maximum ctx size (" << n_ctx_ << ")\n";
            std::exit(EXIT_FAILURE);
        }
        // one new row: the fused decode path (same bytes, 6 launches per block)
        if (fast_decode_ && tokens.numel() - start_pos == 1 && tokens.is_host_external()) {
            const int n = tokens.numel();
            const int32_t* ids = static_cast<const int32_t*>(tokens.host_external_ptr());
            decode_set_tokens(ids + (n - 1), n - 1, 1);
            decode_step(n, /*use_graph=*/true);
            (void)lm_head_.acv.device_ptr_mut();      // the step wrote the logits in HBM: host mirror is stale
            return lm_head_.acv;
        }
        return lm_head_.forward(final_rows(tokens, start_pos));
    }

    // rows [start_pos, n) through the blocks and the final norm, operator by operator (this class drives its own decoder
    // above; with the fast path switched off the modules must not record the row for theirs either -- gten/modules.h)
    // (n_blocks >= 0: only the first n_blocks blocks run, the final norm behind them -- include/gten_host_embed.h, `layer`)
    Tensor final_rows(const Tensor& tokens, const int start_pos, const int n_blocks = -1)
    {
        struct OpsOnly {
            bool was = detail::fused_rows_enabled();
            OpsOnly() { detail::fused_rows_enabled() = false; }
            ~OpsOnly() { detail::fused_rows_enabled() = was; }
        } ops_only;
        Tensor x = tok_emb_.forward(tokens, start_pos);
        for (size_t i = 0; i < blocks_in(n_blocks); i++) x = blocks_[i].forward(x, start_pos);
        return norm_.forward(x, start_pos);
    }

    // ---- several prompts as ONE row matrix (TinyLlamaBatch::prefill_many; include/gten_hip.h, gten_hip_set_row_segments):
    // rows [starts[k], starts[k + 1]) of `tokens` are prompt k.  Returns the final-norm rows; logits_of_row gives the
    // logits of one of them.  This object's K / V tensors then hold every prompt's rows, at the prompt's rows.
    Tensor hidden_rows(const Tensor& tokens, const std::vector<int32_t>& starts, const int n_blocks = -1)
    {
        GTEN_ASSERTM(tokens.numel() <= n_ctx_ && (int)starts.size() >= 2 && starts.back() == tokens.numel(), "hidden_rows: %d rows, context %d",
                     tokens.numel(), n_ctx_);
        struct OpsOnly {
            bool was = detail::fused_rows_enabled();
            OpsOnly() { detail::fused_rows_enabled() = false; }
            ~OpsOnly() { detail::fused_rows_enabled() = was; }
        } ops_only;
        struct Segments {
            explicit Segments(const std::vector<int32_t>& s) { GTEN_HIP_OK(gten_hip_set_row_segments(s.data(), (int)s.size() - 1)); }
            ~Segments() { gten_hip_set_row_segments(nullptr, 0); }
        } segments(starts);
        Tensor x = tok_emb_.forward(tokens, 0);
        for (size_t i = 0; i < blocks_in(n_blocks); i++) x = blocks_[i].forward(x, 0);
        return norm_.forward(x, 0);
    }
    // hidden_rows for prompts that all begin with the SAME prefix_len ids (include/gten_hip_prefix.h): `tokens`
    // holds only what follows the prefix in each prompt, `prefix` is the model object whose K / V tensors hold the prefix's
    // rows [0, prefix_len).  This object's K / V tensors then hold the prompts' remaining rows, at their rows of the matrix.
    Tensor hidden_rows_prefixed(const Tensor& tokens, const std::vector<int32_t>& starts, TinyLlama& prefix, int prefix_len)
    {
        struct Scope {
            detail::PrefixedRows& pr = detail::prefixed_rows();
            Scope(TinyLlama& m, int len)
            {
                GTEN_ASSERTM(pr.call && len > 0, "hidden_rows_prefixed: no device entry point installed (prefix %d)", len);
                pr.kv.clear();
                for (auto& blk : m.blocks_) pr.kv.push_back({blk.attn.key.acv.device_ptr(), blk.attn.value.acv.device_ptr()});
                pr.layer = 0;
                pr.len = len;
            }
            ~Scope() { pr.len = 0; pr.kv.clear(); }
        } scope(prefix, prefix_len);
        return hidden_rows(tokens, starts);
    }
    // hidden_rows for prompts that each CONTINUE A CONTEXT OF THEIR OWN (include/gten_hip_continue.h): segment s of
    // `tokens` holds the ids of positions ctx_len[s] .., `ctx[s]` is the model object whose K / V tensors hold that segment's rows
    // [0, ctx_len[s]).  This object's K / V tensors then hold the new rows, at their rows of the matrix.
    Tensor hidden_rows_continued(const Tensor& tokens, const std::vector<int32_t>& starts, const std::vector<TinyLlama*>& ctx, const std::vector<int>& ctx_len)
    {
        struct Scope {
            detail::ContinuedRows& cr = detail::continued_rows();
            Scope(const std::vector<TinyLlama*>& ctx, const std::vector<int>& len, int n_layers)
            {
                GTEN_ASSERTM(cr.set && cr.call && !ctx.empty() && ctx.size() == len.size(), "hidden_rows_continued: no device entry point installed (%zu contexts)", ctx.size());
                cr.n_layers = n_layers;
                cr.n_segments = (int)ctx.size();
                cr.ctx.clear();
                for (int l = 0; l < n_layers; l++)
                    for (size_t s = 0; s < ctx.size(); s++) {
                        AttentionBlock& blk = ctx[s]->blocks_[(size_t)l];
                        cr.ctx.push_back(gten_hip_row_ctx{blk.attn.key.acv.device_ptr(), blk.attn.value.acv.device_ptr(), len[s]});
                    }
                cr.layer = 0;
                cr.on = true;
            }
            ~Scope()
            {
                cr.on = false;
                cr.ctx.clear();
                cr.set(nullptr, 0, 0);
            }
        } scope(ctx, ctx_len, params.n_layers);
        GTEN_ASSERTM(starts.size() == ctx.size() + 1, "hidden_rows_continued: %zu segments, %zu contexts", starts.size() - 1, ctx.size());
        return hidden_rows(tokens, starts);
    }
    Tensor logits_of_row(const Tensor& hidden, int row)
    {
        Tensor v = hidden;                                    // (a shallow handle: the same storage, its own shape)
        v.resize({row + 1, params.n_embd});
        return lm_head_.forward(v);                           // EmbeddingLinear computes the last row of what it is given
    }
    AttentionBlock& block(int i) { return blocks_[(size_t)i]; }
    size_t blocks_in(int n_blocks) const { return n_blocks < 0 ? blocks_.size() : std::min(blocks_.size(), (size_t)n_blocks); }
    // the second TinyLlama of kScoreRows rows that aliases these weights: the segmented-prompt model of score_many, which
    // creates it in the same way on first use (host/capi_embed.cpp runs its grouped texts on it)
    TinyLlama& segment_model()
    {
        if (!pre_) {
            pre_.reset(new TinyLlama(kScoreRows, dtype_, params));
            pre_->set_fast_decode(false);
            for (int w = 0; w < n_weights(); w++) pre_->weight(w) = weight(w);
        }
        return *pre_;
    }

    // ---- scoring given ids (include/gten_host_score.h): the lm_head over EVERY computed row, in chunks of
    // at most kScoreChunk rows into an f32 scratch this object owns (row pitch padded to 16 bytes), each chunk read by
    // gten_hip_row_logprobs.  Chunks start at the first row of a text, so a row's logits depend on the text alone.
    static constexpr int kScoreChunk = 512;
    static constexpr int kScoreRows = 4096;    // rows of one score_many group (GTEN_SEG_MAX_ROWS)
    static constexpr int kScoreTexts = 32;     // texts of one score_many group
    long long score_stride() const { return ((long long)params.n_vocab + 3) & ~3LL; }

    // the lm_head of rows [0, rows) of x (dtype code xdt, pitch bytes), handed chunk by chunk to fn(logits, first row, rows, stride)
    template <class Fn>
    void lm_head_rows(const void* x, int xdt, size_t pitch, int rows, Fn fn)
    {
        const long long stride = score_stride();
        if (!score_logits_) GTEN_HIP_OK(gten_hip_malloc(&score_logits_, (size_t)kScoreChunk * (size_t)stride * sizeof(float)));
        for (int r0 = 0; r0 < rows; r0 += kScoreChunk) {
            const int cr = std::min(kScoreChunk, rows - r0);
            GTEN_HIP_OK(gten_hip_matmul_2d((const uint8_t*)x + (size_t)r0 * pitch, xdt, pitch, lm_head_.weight.device_weight(),
                                           dtype_code(dtype_.wdtype), score_logits_, GTEN_F32, (size_t)stride * sizeof(float), cr,
                                           params.n_embd, params.n_vocab, 0));
            fn((const float*)score_logits_, r0, cr, stride);
        }
    }
    // rows [start_pos, n) of tokens computed as logits() computes them, their lm_head handed to fn as above (one new row on
    // the fused decoder: its logits buffer is the row)
    template <class Fn>
    void rows_logits(const Tensor& tokens, const int start_pos, Fn fn)
    {
        const int rows = tokens.numel() - start_pos;
        if (fast_decode_ && rows == 1 && tokens.is_host_external()) {
            const Tensor lg = logits(tokens, start_pos);
            fn((const float*)lg.device_ptr(), 0, 1, (long long)params.n_vocab);
            return;
        }
        const Tensor h = final_rows(tokens, start_pos);
        const size_t pitch = (size_t)h.bstride(0);
        lm_head_rows((const uint8_t*)h.device_ptr() + (size_t)start_pos * pitch, dtype_code(h.dtype()), pitch, rows, fn);
    }
    // ... scored against targets already on the device (one per row); log-probs and ranks into lp / rk on the device
    void score_dev(const Tensor& tokens, const int start_pos, const int32_t* tdev, float* lp, int32_t* rk)
    {
        rows_logits(tokens, start_pos, [&](const float* lg, int r0, int cr, long long stride) {
            GTEN_HIP_OK(gten_hip_row_logprobs(lg, cr, params.n_vocab, stride, tdev + r0, lp + r0, rk + r0, nullptr));
        });
    }
    // gten_host_model_score: targets (host) -> log-probs / ranks (host; rank_host may be null), one copy back at the end
    void score(const Tensor& tokens, const int start_pos, const int32_t* targets, float* lp_host, int32_t* rank_host)
    {
        const int rows = tokens.numel() - start_pos;
        int32_t* io = score_io(rows);
        GTEN_HIP_OK(gten_hip_memcpy_h2d(io, targets, (size_t)rows * sizeof(int32_t)));
        score_dev(tokens, start_pos, io, (float*)(io + rows), io + 2 * rows);
        score_copy_back(io + rows, rows, lp_host, rank_host);
    }
    // gten_host_model_logits_all: f32 [n - start_pos][n_vocab] on the host
    void logits_all(const Tensor& tokens, const int start_pos, float* out)
    {
        const int V = params.n_vocab;
        std::vector<float> stage;
        rows_logits(tokens, start_pos, [&](const float* lg, int r0, int cr, long long stride) {
            stage.resize((size_t)cr * (size_t)stride);
            GTEN_HIP_OK(gten_hip_memcpy_d2h(stage.data(), lg, stage.size() * sizeof(float)));
            for (int r = 0; r < cr; r++) std::memcpy(out + (size_t)(r0 + r) * V, stage.data() + (size_t)r * stride, (size_t)V * sizeof(float));
        });
    }
    // gten_host_model_score_many: text k = tokens[starts[k] .. starts[k + 1]) (1 .. min(2048, context) ids each), scored from
    // position 0.  Texts of 16..2048 ids share row-segment groups (hidden_rows on a second TinyLlama of kScoreRows rows that
    // aliases these weights) of at most kScoreTexts texts / kScoreRows rows, formed in order; the lm_head then runs per text.
    // Other texts -- or all of them, where the configuration has no segmented prompt path -- go one by one through score_dev.
    void score_many(const int32_t* tokens, const int32_t* starts, int n_texts, const int32_t* targets, float* lp_host, int32_t* rank_host)
    {
        const int total = starts[n_texts];
        int32_t* io = score_io(total);
        GTEN_HIP_OK(gten_hip_memcpy_h2d(io, targets, (size_t)total * sizeof(int32_t)));
        float* lp = (float*)(io + total);
        int32_t* rk = io + 2 * total;
        const bool seg = gten_hip_row_segments_ok(params.n_embd, params.n_ffn, params.n_heads, params.n_query_groups,
                                                  dtype_code(dtype_.wdtype), dtype_code(dtype_.adtype)) == 1;
        std::vector<int> group;
        int group_rows = 0;
        auto flush = [&]() {
            if (group.empty()) return;
            if (!pre_) {
                pre_.reset(new TinyLlama(kScoreRows, dtype_, params));
                pre_->set_fast_decode(false);
                for (int w = 0; w < n_weights(); w++) pre_->weight(w) = weight(w);
            }
            std::vector<int32_t> ids, st{0};
            for (int k : group) {
                ids.insert(ids.end(), tokens + starts[k], tokens + starts[k + 1]);
                st.push_back((int32_t)ids.size());
            }
            Tensor tk(ids.data(), {(int)ids.size()}, kInt32);
            const Tensor h = pre_->hidden_rows(tk, st);
            const size_t pitch = (size_t)h.bstride(0);
            const uint8_t* hp = (const uint8_t*)h.device_ptr();
            for (size_t g = 0; g < group.size(); g++) {
                const int off = starts[group[g]];
                lm_head_rows(hp + (size_t)st[g] * pitch, dtype_code(h.dtype()), pitch, st[g + 1] - st[g],
                             [&](const float* lg, int r0, int cr, long long stride) {
                                 GTEN_HIP_OK(gten_hip_row_logprobs(lg, cr, params.n_vocab, stride, io + off + r0, lp + off + r0, rk + off + r0, nullptr));
                             });
            }
            group.clear();
            group_rows = 0;
        };
        for (int k = 0; k < n_texts; k++) {
            const int len = starts[k + 1] - starts[k];
            if (!seg || len < 16 || len > 2048) {
                Tensor tk(tokens + starts[k], {len}, kInt32);
                score_dev(tk, 0, io + starts[k], lp + starts[k], rk + starts[k]);
                continue;
            }
            if ((int)group.size() == kScoreTexts || group_rows + len > kScoreRows) flush();
            group.push_back(k);
            group_rows += len;
        }
        flush();
        score_copy_back(io + total, total, lp_host, rank_host);
    }

    // ---- single-token decode fast path (include/gten_hip.h, "decode fast path")
    void set_fast_decode(bool on) { fast_decode_ = on; }
    bool fast_decode() const { return fast_decode_; }

    // token ids for positions [first, first+count) of the sequence being decoded
    void decode_set_tokens(const int32_t* ids, int first, int count)
    {
        ensure_decoder();
        GTEN_HIP_OK(gten_hip_decoder_set_tokens(dec_, ids, first, count));
    }
    // asynchronous: row n-1 -> logits (lm_head_.acv, in HBM) and their argmax
    void decode_step(int n, bool use_graph)
    {
        ensure_decoder();
        GTEN_HIP_OK(gten_hip_decoder_step(dec_, n, use_graph ? 1 : 0));
    }
    // asynchronous: `count` consecutive rows n_first - 1, n_first, ... (ids on the device), four steps per graph replay
    void decode_steps(int n_first, int count, bool use_graph)
    {
        ensure_decoder();
        GTEN_HIP_OK(gten_hip_decoder_steps(dec_, n_first, count, use_graph ? 1 : 0));
    }
    // device pointers of this model's weights / logits buffer for a decoder (shared code with TinyLlamaBatch)
    void describe(gten_hip_decoder_desc* d, std::vector<gten_hip_layer_ptrs>* L)
    {
        *d = gten_hip_decoder_desc{};
        d->n_vocab = params.n_vocab; d->max_ctx = n_ctx_; d->n_embd = params.n_embd; d->n_ffn = params.n_ffn;
        d->n_layers = params.n_layers; d->n_heads = params.n_heads; d->n_kv_heads = params.n_query_groups;
        d->wdtype = dtype_code(dtype_.wdtype); d->adtype = dtype_code(dtype_.adtype);
        d->embed = tok_emb_.weight.device_weight();
        d->final_norm = norm_.weight.device_weight();
        d->lm_head = lm_head_.weight.device_weight();
        d->logits = static_cast<float*>(lm_head_.acv.device_ptr_mut());
        L->assign((size_t)params.n_layers, gten_hip_layer_ptrs{});
        for (int i = 0; i < params.n_layers; i++) {
            AttentionBlock& b = blocks_[(size_t)i];
            gten_hip_layer_ptrs& p = (*L)[(size_t)i];
            p.wq = b.attn.query.weight.device_weight();
            p.wk = b.attn.key.weight.device_weight();
            p.wv = b.attn.value.weight.device_weight();
            p.wo = b.attn.qkv_proj.weight.device_weight();
            p.wgate = b.ffn_gate_proj.weight.device_weight();
            p.wup = b.ffn_up_proj.weight.device_weight();
            p.wdown = b.ffn_down_proj.weight.device_weight();
            p.attn_norm = b.attn_norm.weight.device_weight();
            p.ffn_norm = b.ffn_norm.weight.device_weight();
            p.kcache = b.attn.key.acv.device_ptr_mut();      // the K/V caches ARE these activation tensors
            p.vcache = b.attn.value.acv.device_ptr_mut();
        }
    }

    // HIP-event timed replay of one kernel family of the decode step (bench.py roofline)
    double decode_time_family(int family, int n, int reps, int* launches)
    {
        ensure_decoder();
        double us = 0.0;
        // (a family this decoder's step does not launch is reported, not fatal: < 0)
        if (gten_hip_decoder_time_family(dec_, family, n, reps, &us, launches) != 0) return -1.0;
        return us;
    }
    int decode_result(int n)
    {
        ensure_decoder();
        int32_t tok = -1;
        GTEN_HIP_OK(gten_hip_decoder_result(dec_, n, &tok));
        return tok;
    }
    // greedy generation with the sampler on the device (gten_hip_decoder_generate): ids [0, n_first) are known, the
    // caches hold rows [0, n_first - 1); returns the number of new ids written to `out`
    int decode_generate(const int32_t* ids, int n_first, int max_new, int eos, int32_t* out)
    {
        decode_set_tokens(ids, 0, n_first);
        int got = 0;
        GTEN_HIP_OK(gten_hip_decoder_generate(dec_, n_first, max_new, eos, out, &got));
        (void)lm_head_.acv.device_ptr_mut();          // the steps wrote logits in HBM: host mirror is stale
        return got;
    }

    // the fused decoder itself, for what sets requests on it (host/generate.h, host/capi_bias.cpp, host/capi_logprobs.cpp)
    gten_hip_decoder* decoder_handle()
    {
        ensure_decoder();
        return dec_;
    }

    ~TinyLlama()
    {
        if (dec_) gten_hip_decoder_destroy(dec_);
        if (score_logits_) gten_hip_free(score_logits_);
        if (score_io_) gten_hip_free(score_io_);
    }
    TinyLlama(const TinyLlama&) = delete;
    TinyLlama& operator=(const TinyLlama&) = delete;

    int n_weights() const { return 1 + 9 * params.n_layers + 2; }

    // weight tensors in .gten order (tinyllama.cpp:345-391)
    Tensor& weight(int idx)
    {
        const int last = n_weights() - 1;
        GTEN_ASSERT(idx >= 0 && idx <= last);
        if (idx == 0) return tok_emb_.weight;
        if (idx == last) return lm_head_.weight;
        if (idx == last - 1) return norm_.weight;
        AttentionBlock& b = blocks_[(idx - 1) / 9];
        switch ((idx - 1) % 9) {
        case 0: return b.attn.query.weight;
        case 1: return b.attn.key.weight;
        case 2: return b.attn.value.weight;
        case 3: return b.attn.qkv_proj.weight;
        case 4: return b.ffn_gate_proj.weight;
        case 5: return b.ffn_up_proj.weight;
        case 6: return b.ffn_down_proj.weight;
        case 7: return b.attn_norm.weight;
        default: return b.ffn_norm.weight;
        }
    }

    // .gten reader (tinyllama.cpp:301-392): magic, then per tensor
    // [i32 len][name][i32 len][name][i32 nbytes][payload] in fixed order; names
    // are skipped, the payload size must match the tensor.
    void load_from_ckpt(std::ifstream& ckpt)
    {
        Timer load_timer{&load_time};
        int64_t magic = 0;
        ckpt.read(reinterpret_cast<char*>(&magic), sizeof(magic));
        GTEN_ASSERTM(magic == 0x454c49464e455447LL, "Magic number in the binary does not match the expected one.");
        for (int i = 0; i < n_weights(); i++) {
            std::string name;
            for (int rep = 0; rep < 2; rep++) {
                int32_t len = 0;
                ckpt.read(reinterpret_cast<char*>(&len), sizeof(len));
                GTEN_ASSERTM(ckpt.good() && len >= 0 && len < 4096, "Corrupt tensor header in checkpoint.");
                name.resize((size_t)len);
                ckpt.read(name.data(), len);
            }
            int32_t nbytes = 0;
            ckpt.read(reinterpret_cast<char*>(&nbytes), sizeof(nbytes));
            Tensor& w = weight(i);
            GTEN_ASSERTM(static_cast<size_t>(nbytes) == w.nbytes(), "Weight `%s` data size: %d does not match the expected size: %zu.",
                         name.c_str(), nbytes, w.nbytes());
            ckpt.read(w.data_ptr<char>(), nbytes);      // host mirror; staged to HBM below
            GTEN_ASSERTM(ckpt.good(), "Checkpoint ended inside weight `%s`.", name.c_str());
            w.device_weight();                          // upload (+ repack Q8/Q4) and drop the host copy
        }
    }

    // Synthetic weights (host/synth.h): generated, quantized like the reference
    // converter, and staged to HBM tensor by tensor.
    // GTEN_SYNTH_CACHE_DIR (bench.py --gpus N sets it to /dev/shm): the replicas of one node generate the synthetic weights
    // ONCE -- the first process to create the lock file generates them (OpenMP over all cores, seconds) and publishes the
    // file with a rename, the others wait for it and read it -- instead of N OpenMP generations at the same time.
    void load_synthetic(uint64_t seed)
    {
        Timer load_timer{&load_time};
        const char* dir = std::getenv("GTEN_SYNTH_CACHE_DIR");
        if (dir && dir[0] && load_synthetic_cached(dir, seed)) return;
        std::vector<float> f32;
        for (int i = 0; i < n_weights(); i++) {
            Tensor& w = weight(i);
            synth_weight_bytes(params, dtype_, seed, i, f32, w.data_ptr<uint8_t>(), w.nbytes());
            w.device_weight();
        }
    }

    bool load_synthetic_cached(const char* dir, uint64_t seed)
    {
        size_t total = 0;
        for (int i = 0; i < n_weights(); i++) total += weight(i).nbytes();
        char base[512];
        std::snprintf(base, sizeof(base), "%s/gten_synth_v%d_s%llu_w%d_a%d_e%d_f%d_l%d_v%d_h%d_g%d.bin", dir, synth::kFormat, (unsigned long long)seed,
                      (int)dtype_.wdtype, (int)dtype_.adtype, params.n_embd, params.n_ffn, params.n_layers, params.n_vocab, params.n_heads,
                      params.n_query_groups);
        const std::string path = base, lock = path + ".lock", tmp = path + ".tmp";
        auto ready = [&]() { struct stat st; return ::stat(path.c_str(), &st) == 0 && (size_t)st.st_size == total; };
        if (!ready()) {
            // an advisory lock on the lock FILE (never its existence): a generator that dies releases it, nobody waits for a
            // stale file.  Whoever gets the exclusive lock generates; the others block on a shared lock until it is done.
            const int fd = ::open(lock.c_str(), O_CREAT | O_RDWR, 0644);
            if (fd < 0) return false;
            if (::flock(fd, LOCK_EX | LOCK_NB) == 0) {
                if (!ready()) {                                  // (it may have been finished between the check and the lock)
                    const int omp_before = omp_get_max_threads();
                    if (const char* nt = std::getenv("GTEN_SYNTH_GEN_THREADS")) {
                        const int n = std::atoi(nt);
                        if (n > 0) omp_set_num_threads(n);       // the other replicas only wait: every core for this one
                    }
                    std::FILE* f = std::fopen(tmp.c_str(), "wb");
                    bool ok = f != nullptr;
                    std::vector<float> f32;
                    for (int i = 0; i < n_weights(); i++) {
                        Tensor& w = weight(i);
                        synth_weight_bytes(params, dtype_, seed, i, f32, w.data_ptr<uint8_t>(), w.nbytes());
                        if (ok) ok = std::fwrite(w.data_ptr<uint8_t>(), 1, w.nbytes(), f) == w.nbytes();
                        w.device_weight();
                    }
                    if (f) ok = (std::fclose(f) == 0) && ok;
                    if (ok) std::rename(tmp.c_str(), path.c_str());
                    else std::remove(tmp.c_str());
                    omp_set_num_threads(omp_before);             // (the generation is over: this replica's share of the cores again)
                    ::flock(fd, LOCK_UN);
                    ::close(fd);
                    return true;
                }
                ::flock(fd, LOCK_UN);
            } else {
                ::flock(fd, LOCK_SH);                            // blocks while the generator works
                ::flock(fd, LOCK_UN);
            }
            ::close(fd);
            if (!ready()) return false;                          // (the generator could not write the file: everybody for themselves)
        }
        std::FILE* f = std::fopen(path.c_str(), "rb");
        if (!f) return false;
        bool ok = true;
        for (int i = 0; i < n_weights() && ok; i++) {
            Tensor& w = weight(i);
            ok = std::fread(w.data_ptr<uint8_t>(), 1, w.nbytes(), f) == w.nbytes();
            if (ok) w.device_weight();
        }
        std::fclose(f);
        return ok;                                               // (a short read: the caller generates everything again)
    }

    // shape of tensor idx: rows, cols, storage dtype
    static void weight_shape(const TinyLLamaParams& p, ModuleDtype md, int idx, int* rows, int* cols, Dtype* dt)
    {
        const int E = p.n_embd, F = p.n_ffn, V = p.n_vocab, KV = (E / p.n_heads) * p.n_query_groups;
        const int last = 1 + 9 * p.n_layers + 1;
        *dt = md.wdtype;
        if (idx == 0 || idx == last) { *rows = V; *cols = E; return; }
        if (idx == last - 1) { *rows = 1; *cols = E; *dt = kFloat16; return; }
        switch ((idx - 1) % 9) {
        case 0: case 3: *rows = E; *cols = E; break;
        case 1: case 2: *rows = KV; *cols = E; break;
        case 4: case 5: *rows = F; *cols = E; break;
        case 6: *rows = E; *cols = F; break;
        default: *rows = 1; *cols = E; *dt = kFloat16; break;
        }
    }

    static void synth_weight_bytes(const TinyLLamaParams& p, ModuleDtype md, uint64_t seed, int idx,
                                   std::vector<float>& scratch, uint8_t* out, size_t nbytes)
    {
        int rows, cols;
        Dtype dt;
        weight_shape(p, md, idx, &rows, &cols, &dt);
        GTEN_ASSERTM((size_t)rows * synth::row_bytes(dt, cols) == nbytes, "synthetic weight %d: size mismatch", idx);
        const bool is_norm = (rows == 1 && dt == kFloat16);
        scratch.resize((size_t)rows * cols);
        synth::fill_normal(scratch.data(), scratch.size(), seed, (uint64_t)idx, is_norm ? 1.0f : 0.0f, is_norm ? 0.05f : 0.02f);
        synth::quantize_weight(scratch.data(), rows, cols, dt, out);
    }

    // Lin / Attn / Other split in the spirit of tinyllama.cpp:515-582.  The times
    // are meaningful only with GTEN_HIP_SYNC_TIMERS=1 (see gten/modules.h).
    void print_perf(const int n_pred_tokens)
    {
        int64_t lin = lm_head_.exec_time, attn = 0, other = tok_emb_.exec_time + norm_.exec_time;
        for (auto& b : blocks_) {
            lin += b.attn.query.exec_time + b.attn.key.exec_time + b.attn.value.exec_time + b.attn.qkv_proj.exec_time +
                   b.ffn_gate_proj.exec_time + b.ffn_up_proj.exec_time + b.ffn_down_proj.exec_time;
            attn += b.attn.exec_time_attn;
            other += b.attn_norm.exec_time + b.ffn_norm.exec_time + b.inp_res.exec_time + b.attn_res.exec_time +
                     b.ffn_mul.exec_time + b.ffn_silu.exec_time + b.attn.q_rope.exec_time + b.attn.k_rope.exec_time;
        }
        const int n = n_pred_tokens > 0 ? n_pred_tokens : 1;
        std::cout << "tokens: " << n_pred_tokens << "  ms/tok: linear " << lin / n << "  attention " << attn / n << "  other "
                  << other / n << "  sample " << sample_time / n << "  load " << load_time << " ms  tensor bytes "
                  << G_TensorMemAllocated / 1000000 << " MB\n";
    }

private:
    Embedding tok_emb_;
    RMSNorm norm_;
    EmbeddingLinear lm_head_;
    std::vector<AttentionBlock> blocks_;
    gten_hip_decoder* dec_ = nullptr;
    bool fast_decode_ = [] { const char* e = std::getenv("GTEN_HIP_FAST_DECODE"); return !(e && e[0] == '0'); }();
    // scoring (allocated on first use): the lm_head chunk [kScoreChunk][score_stride()] f32, the per-call device words
    // [targets][log-probs][ranks], and the segmented-prompt model of score_many
    void* score_logits_ = nullptr;
    void* score_io_ = nullptr;
    size_t score_io_bytes_ = 0;
    std::unique_ptr<TinyLlama> pre_;

    int32_t* score_io(int rows)
    {
        const size_t need = (size_t)rows * 3 * sizeof(int32_t);
        if (need > score_io_bytes_) {
            if (score_io_) GTEN_HIP_OK(gten_hip_free(score_io_));
            score_io_ = nullptr;
            GTEN_HIP_OK(gten_hip_malloc(&score_io_, need));
            score_io_bytes_ = need;
        }
        return (int32_t*)score_io_;
    }
    // log-probs then ranks, `rows` words each, in ONE copy
    void score_copy_back(const int32_t* dev, int rows, float* lp_host, int32_t* rank_host)
    {
        std::vector<int32_t> got((size_t)rows * 2);
        GTEN_HIP_OK(gten_hip_memcpy_d2h(got.data(), dev, got.size() * sizeof(int32_t)));
        std::memcpy(lp_host, got.data(), (size_t)rows * sizeof(float));
        if (rank_host) std::memcpy(rank_host, got.data() + rows, (size_t)rows * sizeof(int32_t));
    }

    // The decoder works on the SAME HBM tensors the modules own: weights (packed
    // at load), the K/V caches (= attn.key.acv / attn.value.acv) and the logits
    // buffer (= lm_head_.acv); it only adds small per-step scratch of its own.
    void ensure_decoder()
    {
        if (dec_) return;
        gten_hip_decoder_desc d;
        std::vector<gten_hip_layer_ptrs> L;
        describe(&d, &L);
        GTEN_HIP_OK(gten_hip_decoder_create(&d, L.data(), &dec_));
    }

public:
    int64_t load_time = 0;
    int64_t sample_time = 0;
};

// S sequences that share ONE copy of the weights.  Each sequence is a full
// TinyLlama object of the gten API -- its own activation tensors, hence its own K/V caches -- whose
// weight Tensors are shallow copies of sequence 0's (gten Tensors share storage on copy,
// gten/tensor.h:24-29), so the weights exist once in HBM.  Prefill goes through each object's
// operator path; single-token steps of all sequences go through one multi-sequence decoder that
// streams every weight once per step.
namespace detail {
// The shared decoder's prefix entry points (include/gten_hip_prefix_decode.h): decode slots whose caches begin with the shared
// prefix's rows read ONE copy of them.  host/capi_prefix.cpp installs them when the library is loaded -- this header and
// host/capi.cpp name no such symbol, so they go on linking against the test stand-in of include/gten_hip.h alone; without
// them every sequence decodes on its own copy, as before.
struct PrefixDecode {
    int (*prefix_set)(gten_hip_decoder* dec, const gten_hip_kv_ptrs* kv, int prefix_len) = nullptr;
    int (*slot_share)(gten_hip_decoder* dec, int seq, int rows) = nullptr;
    int (*info)(gten_hip_decoder* dec, int seq, int* prefix_len, int* seq_chunks, unsigned long long* prefix_imports,
                unsigned long long* imports_skipping) = nullptr;
};
inline PrefixDecode& prefix_decode()
{
    static PrefixDecode p;
    return p;
}
// ... and the entry points of SEVERAL prefixes (include/gten_hip_prefixes.h), installed by host/capi_prefixes.cpp in the same way.
// Without them only prefix index 0 exists, through the hooks above.
struct PrefixesDecode {
    int (*set)(gten_hip_decoder* dec, int which, const gten_hip_kv_ptrs* kv, int prefix_len) = nullptr;
    int (*share)(gten_hip_decoder* dec, int seq, int which, int rows) = nullptr;
    int (*info)(gten_hip_decoder* dec, int seq, int which, int* seq_which, int* seq_chunks, int* prefix_len, unsigned long long* prefix_imports,
                int* sharers) = nullptr;
};
inline PrefixesDecode& prefixes_decode()
{
    static PrefixesDecode p;
    return p;
}
// ... and the entry points of the GROUP RECORDS (include/gten_hip_groups.h), installed by host/capi_samples.cpp in the same way.
// Without them the members of a sample group decode on their own copies of the prompt's rows.
struct GroupsDecode {
    int (*set)(gten_hip_decoder* dec, int g, const gten_hip_kv_ptrs* kv, int rows) = nullptr;
    int (*share)(gten_hip_decoder* dec, int seq, int g, int rows) = nullptr;
    int (*info)(gten_hip_decoder* dec, int seq, int g, int* seq_group, int* seq_chunks, int* rows, unsigned long long* imports, int* sharers) = nullptr;
};
inline GroupsDecode& groups_decode()
{
    static GroupsDecode p;
    return p;
}
} // namespace detail

constexpr int kGroupsMax = 64;           // group records of a decoder (GTEN_GROUPS_MAX; host/capi_samples.cpp checks that they agree)

// an array with one value per item, or one value for all of them
template <class T>
struct Each {
    const T* each;
    T all;
    T operator[](int j) const { return each ? each[j] : all; }
};

template <class Pick>
class ServeQueue;                        // host/serve.h: the scheduler of TinyLlamaBatch::serve_with

class TinyLlamaBatch {
    template <class Pick>
    friend class ServeQueue;

public:
    TinyLlamaBatch(int n_seq, int n_ctx, ModuleDtype dtype, TinyLLamaParams p = TinyLLamaParams{}) : n_ctx_{n_ctx}, dtype_{dtype}, params_{p}
    {
        GTEN_ASSERTM(n_seq == 2 || n_seq == 4 || n_seq == 8 || (n_seq >= 16 && n_seq <= 64 && n_seq % 16 == 0) || (n_seq > 64 && n_seq <= 256 && n_seq % 64 == 0) ||
                         n_seq == 384 || n_seq == 512,
                     "TinyLlamaBatch: n_seq %d not in {2, 4, 8, 16, 32, 48, 64, 128, 192, 256, 384, 512}", n_seq);
        for (int i = 0; i < n_seq; i++) {
            seqs_.emplace_back(new TinyLlama(n_ctx, dtype, p));
            seqs_.back()->set_fast_decode(false);
        }
    }
    ~TinyLlamaBatch()
    {
        if (dec_) gten_hip_decoder_destroy(dec_);
    }
    TinyLlamaBatch(const TinyLlamaBatch&) = delete;
    TinyLlamaBatch& operator=(const TinyLlamaBatch&) = delete;

    int n_seq() const { return (int)seqs_.size(); }
    TinyLlama& seq(int i) { return *seqs_[(size_t)i]; }
    // cache sets: 0 .. n_seq - 1 are the sequences' own K / V caches, n_seq .. n_seq + spares - 1 the spare ones that serve()
    // fills ahead of the slots that will take them (ensure_spares); prefill / prefill_many take a cache set
    // (sessions, DESIGN.md 3.17: a session's own set has index sess_base() + id, behind room for kSpareCap spares, so that it does
    //  not move when spares grow; n_sets() counts the sets serve() may hand out -- a session's set is never one of them)
    static constexpr int kSpareCap = 512;
    int sess_base() const { return n_seq() + kSpareCap; }
    TinyLlama& cset(int c)
    {
        if (c >= sess_base()) return *sessions_[(size_t)(c - sess_base())].set;
        return c < n_seq() ? *seqs_[(size_t)c] : *spares_[(size_t)(c - n_seq())];
    }
    int n_sets() const { return n_seq() + (int)spares_.size(); }
    int index_space() const { return sessions_.empty() ? n_sets() : sess_base() + (int)sessions_.size(); }
    void ensure_spares(int count)
    {
        GTEN_ASSERTM(count <= kSpareCap, "serve: %d spare cache sets (at most %d)", count, kSpareCap);
        while ((int)spares_.size() < count) {
            spares_.emplace_back(new TinyLlama(n_ctx_, dtype_, params_));
            TinyLlama& m = *spares_.back();
            for (int w = 0; w < seqs_[0]->n_weights(); w++) m.weight(w) = seqs_[0]->weight(w);
        }
    }

    // call after sequence 0's weights are loaded: every other sequence aliases them
    void share_weights()
    {
        for (size_t i = 1; i < seqs_.size(); i++)
            for (int w = 0; w < seqs_[0]->n_weights(); w++) seqs_[i]->weight(w) = seqs_[0]->weight(w);
        pre_.reset();                                        // (the shared prompt matrix aliases the weights too: rebuilt on next use)
        for (Prefix& x : pfx_) { x.set.reset(); x.ids.clear(); }     // (... and the prefix sets, whose rows were computed with the old weights)
        // the shared decoder holds device pointers to the weights and to every cache set it was ever bound to (the spares among
        // them): it goes before they do and is rebuilt on next use
        if (dec_) { GTEN_HIP_OK(gten_hip_decoder_destroy(dec_)); dec_ = nullptr; }
        spares_.clear();                                     // (... and so do the spare cache sets)
        sessions_.clear();                                   // (... and the sessions: their rows were computed with the old weights)
        set_kv_.clear();
        set_share_.clear();
        set_which_.clear();
    }
    void load_synthetic(uint64_t seed)
    {
        seqs_[0]->load_synthetic(seed);
        share_weights();
    }

    // ---- prompt processing.  Wide batches (>= 16 sequences) process prompts of >= 16 ids as segments of ONE row matrix
    // (a scratch model `pre_` on the shared weights; gten_hip_set_row_segments): every projection is one W.x launch for all
    // the prompts of a call, RoPE and attention run per prompt, and each prompt's K / V rows are then copied from the
    // matrix into its slot's caches.  A prompt's bits do not depend on what shares the matrix with it (no K loop is shared
    // between workgroups in segmented calls), so serve(), generate() and prefill() agree whatever they batch together.
    // Up to 8 sequences keep the per-sequence operator path: there the ids are those of a lone TinyLlama, bit for bit.
    static constexpr int kPreRows = 4096;      // rows of the shared matrix (GTEN_SEG_MAX_ROWS; a prompt has at most max_ctx of them)
    static constexpr int kPreMax = 32;         // prompts per call (two copy ranges per prompt and layer: GTEN_HIP_MAX_COPY_RANGES)
    bool batched_prompts() const
    {
        return n_seq() >= 16 && gten_hip_row_segments_ok(params_.n_embd, params_.n_ffn, params_.n_heads, params_.n_query_groups,
                                                         dtype_code(dtype_.wdtype), dtype_code(dtype_.adtype)) == 1;
    }
    // prompts[k] (>= 16 ids each, kPreRows in all, at most kPreMax) onto the caches of sequence slots[k]; first[k] = argmax of
    // prompt k's logits (strict >, first maximum: tinyllama.cpp:416-424); logits_out[k], when given, receives them
    void prefill_many(const std::vector<int>& slots, const std::vector<const std::vector<int32_t>*>& prompts, std::vector<int>* first,
                      std::vector<float*>* logits_out = nullptr, const std::vector<int>* copy_of = nullptr, const std::vector<int>* ctx_of = nullptr)
    {
        prefill_many_with(slots, prompts, first, logits_out, [](int, const float* lg, int n, int32_t* out) {
            GTEN_HIP_OK(gten_hip_argmax_row(lg, n, out));
        }, copy_of, ctx_of);
    }
    // ... with the first id of prompt k (its logits row lg on the device) written to out by pick(k, lg, n_vocab, out)
    // COPIES (sample groups): (*copy_of)[k] = -1: item k is computed, as all are without the list; = c: item k has
    // THE SAME IDS as item c of this call, which is computed (the caller's word: nothing is compared).  A copy adds no rows to the
    // matrix: its set is one more destination of the very ranges item c's set receives -- the prefix rows in front where c takes
    // a registered prefix's short way, then c's own rows out of the matrix -- and carries the same marks; its first id is drawn
    // by pick(k, ...) from c's logits row while that row is alive.  kPreMax and kPreRows count computed prompts only.
    // CONTINUED ITEMS (extend_many): (*ctx_of)[k] = 0: item k is a whole prompt, as all are without the list; = n > 0:
    // set slots[k] keeps its rows [0, n) and prompts[k] holds the ids of positions n ..: the continued items are one row matrix
    // of their new rows behind contexts of their own (hidden_rows_continued), the new K / V rows go into the sets at [n, n + rows).
    // A continued item may hold fewer than 16 ids (at least 1): its segment is filled up to 16 rows behind them (extend_group).
    // A continued item is never a copy and never copied.
    template <class Pick>
    void prefill_many_with(const std::vector<int>& slots, const std::vector<const std::vector<int32_t>*>& prompts, std::vector<int>* first,
                           std::vector<float*>* logits_out, Pick pick, const std::vector<int>* copy_of = nullptr, const std::vector<int>* ctx_of = nullptr)
    {
        const int K = (int)slots.size();
        GTEN_ASSERTM(K >= 1 && prompts.size() == slots.size() && (!copy_of || copy_of->size() == slots.size()) && (!ctx_of || ctx_of->size() == slots.size()),
                     "prefill_many: %d prompts", K);
        auto ctx_at = [&](int k) { return ctx_of ? (*ctx_of)[(size_t)k] : 0; };
        int computed = 0;
        std::vector<std::vector<int>> copies((size_t)K);               // per computed item: the items that copy it
        for (int k = 0; k < K; k++) {
            const int c = copy_of ? (*copy_of)[(size_t)k] : -1;
            if (c < 0) { computed++; continue; }
            GTEN_ASSERTM(c < K && c != k && (*copy_of)[(size_t)c] < 0 && prompts[(size_t)c]->size() == prompts[(size_t)k]->size() && ctx_at(k) == 0 && ctx_at(c) == 0,
                         "prefill_many: item %d copies item %d", k, c);
            copies[(size_t)c].push_back(k);
        }
        GTEN_ASSERTM(computed >= 1 && computed <= kPreMax, "prefill_many: %d prompts to compute (at most %d)", computed, kPreMax);
        ensure_pre();
        for (int k = 0; k < K; k++)
            GTEN_ASSERTM((int)prompts[(size_t)k]->size() >= (ctx_at(k) > 0 ? 1 : 16) && ctx_at(k) >= 0 && ctx_at(k) + (int)prompts[(size_t)k]->size() <= n_ctx_,
                         "prefill_many: a prompt of %zu ids behind %d rows", prompts[(size_t)k]->size(), ctx_at(k));
        first->assign((size_t)K, 0);
        // a prompt's first id: its logits row stays on the device and so does the sampler (gten_hip_argmax_row, the greedy rule
        // of tinyllama.cpp:416-424) -- the K ids come back in ONE 4 K-byte copy and one wait instead of K copies of 128 KB, K
        // waits and K host loops over the vocabulary (round 4); a caller that wants a prompt's logits gets them as before
        // (one word per ITEM of the call, copies included)
        if (!first_ids_ || first_ids_->numel() < K) first_ids_.reset(new Tensor({std::max(K, kPreMax)}, kInt32));
        int32_t* ids_dev = (int32_t*)first_ids_->device_ptr_mut();
        // the prompts that begin with a registered prefix (set_prefix_at; the longest one, prefix_of) are one row matrix per prefix
        // of what follows it, the others one of whole prompts: one call per group
        std::vector<int> group[kPrefixesMax + 1], continued;
        for (int k = 0; k < K; k++) {
            if (ctx_at(k) > 0) continued.push_back(k);
            else if (!copy_of || (*copy_of)[(size_t)k] < 0) group[prefix_of(*prompts[(size_t)k]) + 1].push_back(k);
        }
        if (!continued.empty()) extend_group(continued, slots, prompts, *ctx_of, logits_out, ids_dev, pick);
        for (int w = 0; w < kPrefixesMax; w++)
            if (!group[w + 1].empty()) prefill_group(group[w + 1], w, slots, prompts, logits_out, ids_dev, pick, copies);
        if (!group[0].empty()) prefill_group(group[0], -1, slots, prompts, logits_out, ids_dev, pick, copies);
        std::vector<int32_t> got((size_t)K);
        GTEN_HIP_OK(gten_hip_memcpy_d2h(got.data(), ids_dev, (size_t)K * sizeof(int32_t)));
        for (int k = 0; k < K; k++) (*first)[(size_t)k] = got[(size_t)k];
    }

    // ---- a shared prefix (include/gten_host_prefix.h): the ids every later prompt may begin with, processed
    // ONCE onto a cache set of its own.  A prompt that begins with them and has at least 16 ids of its own takes the short
    // way in prefill_many_with: only its own rows are computed (hidden_rows_prefixed), its slot's caches get a copy of the
    // prefix set's K / V rows in front of them.  Same bytes as the whole prompt: rows are independent in segmented calls.
    // 0; -1: bad arguments (16 <= n, n + 17 <= context); -2: this batch does not process prompts as segments
    int set_prefix(const int32_t* tokens, int n) { return set_prefix_at(0, tokens, n); }
    // ... at index `which` of kPrefixesMax (include/gten_host_prefixes.h): every index is a prefix of its own, on a cache set of its
    // own.  Setting, replacing or clearing one leaves the others, the cache sets marked with them and the slots that decode behind
    // them alone.  -1 as well: which outside [0, kPrefixesMax); -2 as well: an index above 0 without the entry points of several
    // prefixes installed.
    int set_prefix_at(int which, const int32_t* tokens, int n)
    {
        if (which < 0 || which >= kPrefixesMax) return -1;
        Prefix& x = pfx_[which];
        if (n == 0) { x.ids.clear(); decoder_prefix(which, false); return 0; }
        if (!tokens || n < 16 || n + 17 > n_ctx_ || n > kPreRows) return -1;
        if (!batched_prompts() || !detail::prefixed_rows().call) return -2;
        if (which > 0 && !detail::prefixes_decode().set) return -2;
        ensure_pre();
        if (!x.set) {
            x.set.reset(new TinyLlama(n_ctx_, dtype_, params_));
            for (int w = 0; w < seqs_[0]->n_weights(); w++) x.set->weight(w) = seqs_[0]->weight(w);
        }
        x.ids.clear();                                         // (nothing shares a half-written set)
        // ... and no decode slot goes on reading the shadow of rows that are about to be replaced: every sequence sharing THIS
        // prefix is back on its own copy before the set is overwritten (the same set is reused in place)
        decoder_prefix(which, false);
        std::vector<int32_t> ids(tokens, tokens + n);
        Tensor tk(ids.data(), {n}, kInt32);
        (void)pre_->hidden_rows(tk, {0, n});
        for (int l = 0; l < params_.n_layers; l++) {
            AttentionBlock& src = pre_->block(l);
            AttentionBlock& dst = x.set->block(l);
            const size_t bytes = (size_t)n * (size_t)src.attn.key.acv.bstride(0);
            const gten_hip_copy_range r[2] = {{dst.attn.key.acv.device_ptr_mut(), src.attn.key.acv.device_ptr(), bytes},
                                              {dst.attn.value.acv.device_ptr_mut(), src.attn.value.acv.device_ptr(), bytes}};
            GTEN_HIP_OK(gten_hip_copy_ranges(r, 2));
        }
        GTEN_HIP_OK(gten_hip_sync());                          // (the set is read from either stream afterwards)
        x.ids = std::move(ids);
        // the decode side: the shared decoder exists from here on, so that every mark made below reaches it at once and whatever
        // writes a marked set's rows afterwards is seen by its watch
        ensure_decoder();
        decoder_prefix(which, true);
        return 0;
    }
    // prefix `which`'s own single-sequence decoder re-decodes rows of its set (tests: a write into a prefix set's rows that the
    // shared decoder hears of through its watch only).  The set no longer holds the registered ids from row n_first - 1 on, so
    // the registration ends on this side: no later prompt takes the short way behind it.  -1: nothing registered there.
    int prefix_set_steps(int which, const int32_t* tokens, int count, int n_first, int steps)
    {
        if (which < 0 || which >= kPrefixesMax || pfx_[which].ids.empty() || !pfx_[which].set) return -1;
        Prefix& x = pfx_[which];
        x.ids.clear();
        forget_prefix_marks(which);
        x.set->decode_set_tokens(tokens, 0, count);
        x.set->decode_steps(n_first, steps, true);
        return 0;
    }
    // the shared decoder's view of several prefixes (gten_hip_decoder_prefixes_info): the prefix sequence seq_i shares (-1: none)
    // and its chunks; prefix `which`'s length there, the imports of its shadow, its sharers.  Without the entry points: -1 / 0.
    void prefixes_decode_info(int seq_i, int which, int* seq_which, int* seq_chunks, int* n_prefix, unsigned long long* prefix_imports, int* sharers)
    {
        if (seq_which) *seq_which = -1;
        if (seq_chunks) *seq_chunks = 0;
        if (n_prefix) *n_prefix = 0;
        if (prefix_imports) *prefix_imports = 0;
        if (sharers) *sharers = 0;
        if (!detail::prefixes_decode().info) return;
        ensure_decoder();
        GTEN_HIP_OK(detail::prefixes_decode().info(dec_, seq_i, which, seq_which, seq_chunks, n_prefix, prefix_imports, sharers));
    }
    // gten_hip_decoder_prefixes_share on the shared decoder, return code and all (tests: the refusals)
    int prefixes_share_rc(int seq_i, int which, int rows)
    {
        if (!detail::prefixes_decode().share) return 0;
        ensure_decoder();
        return detail::prefixes_decode().share(dec_, seq_i, which, rows);
    }
    int prefix_len_at(int which) const { return (int)pfx_[which].ids.size(); }
    unsigned long long prompts_shared_at(int which) const { return pfx_[which].prompts_shared; }
    unsigned long long rows_computed_at(int which) const { return pfx_[which].rows_computed; }
    // the shared decoder's view (gten_hip_decoder_prefix_info): prefix length it holds, chunks sequence seq_i reads from the
    // prefix shadow, imports of that shadow, sequence imports that skipped shared chunks.  All 0 where nothing is installed.
    void prefix_decode_info(int seq_i, int* n_prefix, int* seq_chunks, unsigned long long* prefix_imports, unsigned long long* imports_skipping)
    {
        if (n_prefix) *n_prefix = 0;
        if (seq_chunks) *seq_chunks = 0;
        if (prefix_imports) *prefix_imports = 0;
        if (imports_skipping) *imports_skipping = 0;
        if (!detail::prefix_decode().info) return;
        ensure_decoder();
        GTEN_HIP_OK(detail::prefix_decode().info(dec_, seq_i, n_prefix, seq_chunks, prefix_imports, imports_skipping));
    }
    // gten_hip_decoder_slot_share on the shared decoder, return code and all (tests: the refusals)
    int slot_share_rc(int seq_i, int rows)
    {
        if (!detail::prefix_decode().slot_share) return 0;
        ensure_decoder();
        return detail::prefix_decode().slot_share(dec_, seq_i, rows);
    }
    // cache set c's rows were written by somebody else than a prompt of this class (gten_host_batch_seq_steps): its mark goes
    void forget_share(int c) { if (c >= 0 && c < (int)set_share_.size()) set_share_[(size_t)c] = 0; }
    int prefix_len() const { return (int)pfx_[0].ids.size(); }
    unsigned long long prompts_shared() const { return pfx_[0].prompts_shared; }
    unsigned long long rows_computed() const { return rows_computed_; }
    // the registered prefix prompt p takes the short way behind (host/prefix_match.h: the longest it begins with and has 16 ids
    // behind); -1: none, the prompt is processed whole
    int prefix_of(const std::vector<int32_t>& p) const
    {
        const int32_t* ids[kPrefixesMax];
        int lens[kPrefixesMax];
        for (int w = 0; w < kPrefixesMax; w++) { ids[w] = pfx_[w].ids.data(); lens[w] = (int)pfx_[w].ids.size(); }
        return prefixes_match_ptrs(ids, lens, kPrefixesMax, p.data(), (int)p.size());
    }
    bool shares_prefix(const std::vector<int32_t>& p) const { return prefix_of(p) >= 0; }
    // rows of the row matrix that prompt p costs
    int computed_rows(const std::vector<int32_t>& p) const
    {
        const int w = prefix_of(p);
        return (int)p.size() - (w >= 0 ? (int)pfx_[w].ids.size() : 0);
    }

private:
    void ensure_pre()
    {
        if (pre_) return;
        pre_.reset(new TinyLlama(kPreRows, dtype_, params_));
        pre_->set_fast_decode(false);
        for (int w = 0; w < seqs_[0]->n_weights(); w++) pre_->weight(w) = seqs_[0]->weight(w);
    }
    // prompts[idx[..]] as ONE row matrix: whole (w < 0, P = 0) or what follows prefix w's P ids
    template <class Pick>
    void prefill_group(const std::vector<int>& idx, int w, const std::vector<int>& slots, const std::vector<const std::vector<int32_t>*>& prompts,
                       std::vector<float*>* logits_out, int32_t* ids_dev, Pick& pick, const std::vector<std::vector<int>>& copies)
    {
        const int P = w >= 0 ? (int)pfx_[w].ids.size() : 0;
        for (int k : idx) {                                    // (sample groups: what the copies of these prompts did not cost)
            samples_copies_ += copies[(size_t)k].size();
            samples_rows_saved_ += copies[(size_t)k].size() * (prompts[(size_t)k]->size() - (size_t)P);
        }
        std::vector<int32_t> ids, starts{0};
        for (int k : idx) {
            const std::vector<int32_t>& p = *prompts[(size_t)k];
            ids.insert(ids.end(), p.begin() + P, p.end());
            starts.push_back((int32_t)ids.size());
        }
        GTEN_ASSERTM((int)ids.size() <= kPreRows, "prefill_many: %zu rows (at most %d)", ids.size(), kPreRows);
        rows_computed_ += ids.size();
        if (P > 0) { pfx_[w].prompts_shared += idx.size(); pfx_[w].rows_computed += ids.size(); }
        Tensor tk(ids.data(), {(int)ids.size()}, kInt32);
        const Tensor hidden = P > 0 ? pre_->hidden_rows_prefixed(tk, starts, *pfx_[w].set, P) : pre_->hidden_rows(tk, starts);
        // every prompt's K / V rows into its own caches (behind a copy of the prefix set's rows when it shares them): one
        // launch per layer, two when the ranges do not fit one
        std::vector<gten_hip_copy_range> ranges;
        auto flush = [&]() {
            if (!ranges.empty()) GTEN_HIP_OK(gten_hip_copy_ranges(ranges.data(), (int)ranges.size()));
            ranges.clear();
        };
        for (int l = 0; l < params_.n_layers; l++) {
            AttentionBlock& src = pre_->block(l);
            const size_t pitch = (size_t)src.attn.key.acv.bstride(0);
            for (size_t i = 0; i < idx.size(); i++) {
                const std::vector<int>& cp = copies[(size_t)idx[i]];
                // (the prompt's own set, then the sets of its copies: further destinations of the same sources)
                for (size_t t = 0; t <= cp.size(); t++) {
                    const int k = t == 0 ? idx[i] : cp[t - 1];
                    if (ranges.size() + (P > 0 ? 4 : 2) > (size_t)GTEN_HIP_MAX_COPY_RANGES) flush();
                    AttentionBlock& dst = cset(slots[(size_t)k]).block(l);
                    uint8_t* dk = (uint8_t*)dst.attn.key.acv.device_ptr_mut();
                    uint8_t* dv = (uint8_t*)dst.attn.value.acv.device_ptr_mut();
                    if (P > 0) {
                        AttentionBlock& pre = pfx_[w].set->block(l);
                        ranges.push_back({dk, pre.attn.key.acv.device_ptr(), (size_t)P * pitch});
                        ranges.push_back({dv, pre.attn.value.acv.device_ptr(), (size_t)P * pitch});
                    }
                    const size_t off = (size_t)starts[i] * pitch, bytes = (size_t)(starts[i + 1] - starts[i]) * pitch;
                    ranges.push_back({dk + (size_t)P * pitch, (const uint8_t*)src.attn.key.acv.device_ptr() + off, bytes});
                    ranges.push_back({dv + (size_t)P * pitch, (const uint8_t*)src.attn.value.acv.device_ptr() + off, bytes});
                }
            }
            flush();
        }
        // "SHARES P ROWS": a set that just received a copy of the prefix rows carries the mark until another prompt is written
        // onto it; outside serve() set c is what sequence c decodes on, and the decoder hears of it now (after the copies above
        // were announced: a later write into the set ends the promise on the decoder's side).  Inside serve() the mark travels
        // with the set and becomes gten_hip_decoder_slot_share when a slot is started on it.
        for (size_t i = 0; i < idx.size(); i++) {
            const std::vector<int>& cp = copies[(size_t)idx[i]];
            for (size_t t = 0; t <= cp.size(); t++) {
                const int c = slots[(size_t)(t == 0 ? idx[i] : cp[t - 1])];
                share_mark(c) = P;
                which_mark(c) = P > 0 ? w : 0;
                if (P > 0 && !in_serve_ && c < n_seq() && dec_) (void)decoder_share(c, w, P);     // (refused -- the sequence is mid-run at a position inside the prefix --: it decodes on its own copy)
            }
        }
        for (size_t i = 0; i < idx.size(); i++) {
            const std::vector<int>& cp = copies[(size_t)idx[i]];
            const Tensor lg = pre_->logits_of_row(hidden, starts[i + 1] - 1);
            // (the copies draw from this row before the next prompt's logits replace it: each with its own request, through pick)
            for (size_t t = 0; t <= cp.size(); t++) {
                const int k = t == 0 ? idx[i] : cp[t - 1];
                pick(k, (const float*)lg.device_ptr(), lg.numel(), ids_dev + k);
                if (logits_out && (*logits_out)[(size_t)k])
                    std::memcpy((*logits_out)[(size_t)k], lg.data_ptr<float>(), (size_t)lg.numel() * sizeof(float));   // (waits for the stream)
            }
        }
    }

    // prompts[idx[..]] as ONE row matrix of new rows, item k behind rows [0, ctx_of[k]) of its own set slots[k].
    // A segment has at least 16 rows (the matrix kernels' shortest): an item of fewer ids is FILLED UP behind its last id with
    // copies of that id.  Rows do not depend on the rows behind them (causal attention; every other kernel works row by row in
    // segmented calls), so the item's own rows hold the bytes of the whole prompt's rows; the fill rows are computed and
    // dropped -- neither copied into the set nor asked for logits.
    static constexpr int kSegMinRows = 16;
    template <class Pick>
    void extend_group(const std::vector<int>& idx, const std::vector<int>& slots, const std::vector<const std::vector<int32_t>*>& prompts,
                      const std::vector<int>& ctx_of, std::vector<float*>* logits_out, int32_t* ids_dev, Pick& pick)
    {
        std::vector<int32_t> ids, starts{0};
        std::vector<TinyLlama*> ctx;
        std::vector<int> len, own;                                  // per item: rows kept, rows of its own in the segment
        for (int k : idx) {
            const std::vector<int32_t>& p = *prompts[(size_t)k];
            ids.insert(ids.end(), p.begin(), p.end());
            if ((int)p.size() < kSegMinRows) ids.insert(ids.end(), (size_t)kSegMinRows - p.size(), p.back());
            starts.push_back((int32_t)ids.size());
            ctx.push_back(&cset(slots[(size_t)k]));
            len.push_back(ctx_of[(size_t)k]);
            own.push_back((int)p.size());
            rows_kept_ += (unsigned long long)ctx_of[(size_t)k];
            rows_computed_ += p.size();
            rows_extended_ += p.size();
        }
        GTEN_ASSERTM((int)ids.size() <= kPreRows, "extend_many: %zu rows (at most %d)", ids.size(), kPreRows);
        turns_continued_ += idx.size();
        Tensor tk(ids.data(), {(int)ids.size()}, kInt32);
        const Tensor hidden = pre_->hidden_rows_continued(tk, starts, ctx, len);
        // the new K / V rows into the sets, behind the rows they continued (announced: a decoder's shadows of these sets re-import)
        std::vector<gten_hip_copy_range> ranges;
        auto flush = [&]() {
            if (!ranges.empty()) GTEN_HIP_OK(gten_hip_copy_ranges(ranges.data(), (int)ranges.size()));
            ranges.clear();
        };
        for (int l = 0; l < params_.n_layers; l++) {
            AttentionBlock& src = pre_->block(l);
            const size_t pitch = (size_t)src.attn.key.acv.bstride(0);
            for (size_t i = 0; i < idx.size(); i++) {
                if (ranges.size() + 2 > (size_t)GTEN_HIP_MAX_COPY_RANGES) flush();
                AttentionBlock& dst = ctx[i]->block(l);
                const size_t at = (size_t)len[i] * pitch, off = (size_t)starts[i] * pitch, bytes = (size_t)own[i] * pitch;
                ranges.push_back({(uint8_t*)dst.attn.key.acv.device_ptr_mut() + at, (const uint8_t*)src.attn.key.acv.device_ptr() + off, bytes});
                ranges.push_back({(uint8_t*)dst.attn.value.acv.device_ptr_mut() + at, (const uint8_t*)src.attn.value.acv.device_ptr() + off, bytes});
            }
            flush();
        }
        // a "shares P rows" mark stays true while the rows written lie behind the prefix's; otherwise it goes
        for (size_t i = 0; i < idx.size(); i++)
            if (int& P = share_mark(slots[(size_t)idx[i]]); P > len[i]) P = 0;
        for (size_t i = 0; i < idx.size(); i++) {
            const int k = idx[i];
            const Tensor lg = pre_->logits_of_row(hidden, starts[i] + own[i] - 1);
            pick(k, (const float*)lg.device_ptr(), lg.numel(), ids_dev + k);
            if (logits_out && (*logits_out)[(size_t)k])
                std::memcpy((*logits_out)[(size_t)k], lg.data_ptr<float>(), (size_t)lg.numel() * sizeof(float));   // (waits for the stream)
        }
    }

public:
    // ---- extend sequences (include/gten_host_sessions.h): set seqs[k] keeps its rows [0, ctx_len[k]) and segment k
    // of the ids becomes positions ctx_len[k] ..; first[k] = argmax of the last new row's logits, logits_out[k] (may be null
    // pointers) receives them.  Where the batch processes prompts as segments and the continued entry points are installed, the
    // segments go as ONE row matrix (several, where they do not fit one) -- those of fewer than 16 ids filled up (extend_group)
    // -- provided history + turn is a prompt the segmented path would take (at least 16 ids in all) and the filled segment
    // ends inside the RoPE table.  The others go one by one through the set's own model object, the way a prompt of fewer
    // than 16 ids goes.  The caller has checked the arguments (host/capi_sessions.cpp).
    // (The fill rows of a short segment sit at positions ctx + n .. ctx + 15, which may lie PAST max_ctx -- prefill_many_with's
    //  assertion speaks of the item's own ids only.  They exist in the row matrix alone, which has kPreRows rows whatever
    //  max_ctx is: they are rotated from the RoPE table, hence the bound kMaxPos, and never written into a cache set.)
    static constexpr int kMaxPos = 2048;       // GTEN_ROPE_MAX_POS
    bool continued_prompts() const { return batched_prompts() && detail::continued_rows().call && detail::continued_rows().set; }
    void extend_many(const std::vector<int>& seqs, const std::vector<int>& ctx_len, const std::vector<std::vector<int32_t>>& tails, std::vector<int>* first,
                     std::vector<float*>* logits_out)
    {
        const int K = (int)seqs.size();
        first->assign((size_t)K, 0);
        const bool many = continued_prompts();
        std::vector<int> slots, ctx, back;
        std::vector<const std::vector<int32_t>*> ps;
        std::vector<float*> lo;
        int rows = 0;
        auto flush = [&]() {
            if (slots.empty()) return;
            std::vector<int> got;
            prefill_many(slots, ps, &got, &lo, nullptr, &ctx);
            for (size_t i = 0; i < back.size(); i++) (*first)[(size_t)back[i]] = got[i];
            slots.clear(); ctx.clear(); back.clear(); ps.clear(); lo.clear();
            rows = 0;
        };
        for (int k = 0; k < K; k++) {
            const int n = (int)tails[(size_t)k].size();
            float* out = logits_out ? (*logits_out)[(size_t)k] : nullptr;
            const int seg = std::max(n, kSegMinRows);
            if (many && ctx_len[(size_t)k] + n >= kSegMinRows && ctx_len[(size_t)k] + seg <= kMaxPos) {
                if ((int)slots.size() == kPreMax || rows + seg > kPreRows) flush();
                slots.push_back(seqs[(size_t)k]); ctx.push_back(ctx_len[(size_t)k]); back.push_back(k); ps.push_back(&tails[(size_t)k]); lo.push_back(out);
                rows += seg;
                continue;
            }
            (*first)[(size_t)k] = extend_one(seqs[(size_t)k], ctx_len[(size_t)k], tails[(size_t)k], out);
        }
        flush();
    }
    // one sequence, operator path on the set's own model object (rows [ctx, ctx + n) are computed, rows [0, ctx) read)
    int extend_one(int c, int ctx, const std::vector<int32_t>& tail, float* logits_out)
    {
        if (int& P = share_mark(c); P > ctx) P = 0;
        std::vector<int32_t> ids((size_t)ctx, 0);                   // (rows [ctx, n) alone are embedded: the earlier ids are not read)
        ids.insert(ids.end(), tail.begin(), tail.end());
        rows_computed_one_ += tail.size();
        Tensor tk(ids.data(), {(int)ids.size()}, kInt32);
        const Tensor lg = cset(c).logits(tk, ctx);
        const float* p = lg.data_ptr<float>();
        int best_i = 0;
        float best = -std::numeric_limits<float>::infinity();
        for (int j = 0; j < lg.numel(); j++)
            if (p[j] > best) { best = p[j]; best_i = j; }
        if (logits_out) std::memcpy(logits_out, p, (size_t)lg.numel() * sizeof(float));
        return best_i;
    }
    // segments that went as continued row matrices, the rows computed for them, the context rows they kept (not recomputed), and
    // the rows of the segments that went one by one -- all since this batch was made
    void extend_info(unsigned long long* turns, unsigned long long* rows, unsigned long long* kept, unsigned long long* rows_one) const
    {
        if (turns) *turns = turns_continued_;
        if (rows) *rows = rows_extended_;
        if (kept) *kept = rows_kept_;
        if (rows_one) *rows_one = rows_computed_one_;
    }
    int max_ctx() const { return n_ctx_; }

    // ---- sessions (include/gten_host_sessions.h): a cache set of its own plus `ids`, the history, and `rows`, the
    // leading positions that have valid K / V.  serve_with's session items decode on it and leave it to the next queue.
    static constexpr int kSessionsMax = 256;
    int sessions_reserve(int n)
    {
        if (n < 0 || n > kSessionsMax) return -1;
        if ((int)sessions_.size() < n) sessions_.resize((size_t)n);
        return 0;
    }
    int session_open()
    {
        for (size_t s = 0; s < sessions_.size(); s++) {
            Session& ss = sessions_[s];
            if (ss.open) continue;
            if (!ss.set) {
                ss.set.reset(new TinyLlama(n_ctx_, dtype_, params_));
                ss.set->set_fast_decode(false);
                for (int w = 0; w < seqs_[0]->n_weights(); w++) ss.set->weight(w) = seqs_[0]->weight(w);
            }
            ss.open = true;
            ss.ids.clear();
            ss.rows = 0;
            share_mark(sess_base() + (int)s) = 0;
            return (int)s;
        }
        return -1;
    }
    bool session_is_open(int s) const { return s >= 0 && s < (int)sessions_.size() && sessions_[(size_t)s].open; }
    int session_close(int s)
    {
        if (!session_is_open(s)) return -1;
        sessions_[(size_t)s].open = false;
        sessions_[(size_t)s].ids.clear();
        sessions_[(size_t)s].rows = 0;
        share_mark(sess_base() + s) = 0;
        return 0;
    }
    const std::vector<int32_t>& session_ids(int s) const { return sessions_[(size_t)s].ids; }
    int session_rows(int s) const { return sessions_[(size_t)s].rows; }
    // the prefix mark the session's set carries: (which, rows), (-1, 0) without one
    void session_prefix(int s, int* which, int* rows)
    {
        const int P = share_mark(sess_base() + s);
        *which = P > 0 ? which_mark(sess_base() + s) : -1;
        *rows = P;
    }
    // the history is cut to n_ids ids; nothing moves on the device (how a caller regenerates or edits the last turn)
    int session_truncate(int s, int n_ids)
    {
        if (!session_is_open(s) || n_ids < 0 || n_ids > (int)sessions_[(size_t)s].ids.size()) return -1;
        sessions_[(size_t)s].ids.resize((size_t)n_ids);
        sessions_[(size_t)s].rows = std::min(sessions_[(size_t)s].rows, n_ids);
        return 0;
    }
    // the session's set was shifted by (keep, drop) on the device (include/gten_host_shift.h; keep + drop <= rows):
    // the history loses ids [keep, keep + drop), `drop` fewer rows are valid, and a prefix mark stays only where keep covers it
    void session_shifted(int s, int keep, int drop)
    {
        Session& ss = sessions_[(size_t)s];
        ss.ids.erase(ss.ids.begin() + keep, ss.ids.begin() + keep + drop);
        ss.rows -= drop;
        if (int& P = share_mark(sess_base() + s); keep < P) P = 0;
    }
    void sessions_info(int* open, unsigned long long* kv_bytes, unsigned long long* turns, unsigned long long* turns_continued,
                       unsigned long long* rows_computed, unsigned long long* rows_kept) const
    {
        int n = 0;
        for (const Session& ss : sessions_) n += ss.open ? 1 : 0;
        const int KV = params_.n_embd / params_.n_heads * params_.n_query_groups;
        if (open) *open = n;
        if (kv_bytes) *kv_bytes = 2ull * (unsigned long long)params_.n_layers * (unsigned long long)n_ctx_ * gten_hip_row_bytes(dtype_code(dtype_.adtype), KV);
        if (turns) *turns = sess_turns_;
        if (turns_continued) *turns_continued = sess_turns_continued_;
        if (rows_computed) *rows_computed = sess_rows_computed_;
        if (rows_kept) *rows_kept = sess_rows_kept_;
    }

    // one prompt onto sequence seq_i's caches; returns the argmax of its logits (logits_out may be null)
    int prefill(int seq_i, const std::vector<int32_t>& prompt, float* logits_out = nullptr)
    {
        if (batched_prompts() && (int)prompt.size() >= 16 && (int)prompt.size() <= kPreRows) {
            std::vector<int> first;
            std::vector<float*> lo{logits_out};
            prefill_many({seq_i}, {&prompt}, &first, &lo);
            return first[0];
        }
        share_mark(seq_i) = 0;
        Tensor tk(prompt.data(), {(int)prompt.size()}, kInt32);
        const Tensor lg = cset(seq_i).logits(tk, 0);                 // operator path on this cache set's own model object
        const float* p = lg.data_ptr<float>();
        int best_i = 0;
        float best = -std::numeric_limits<float>::infinity();
        for (int j = 0; j < lg.numel(); j++)
            if (p[j] > best) { best = p[j]; best_i = j; }
        if (logits_out) std::memcpy(logits_out, p, (size_t)lg.numel() * sizeof(float));
        return best_i;
    }

    // prefill() with the first id chosen on the device by pick(0, logits row in HBM, n_vocab, id out in HBM)
    template <class PickRow>
    int prefill_picked(int seq_i, const std::vector<int32_t>& prompt, PickRow pick)
    {
        if (batched_prompts() && (int)prompt.size() >= 16 && (int)prompt.size() <= kPreRows) {
            std::vector<int> first;
            std::vector<float*> lo{nullptr};
            prefill_many_with({seq_i}, {&prompt}, &first, &lo, pick);
            return first[0];
        }
        share_mark(seq_i) = 0;
        Tensor tk(prompt.data(), {(int)prompt.size()}, kInt32);
        const Tensor lg = cset(seq_i).logits(tk, 0);
        Tensor id({1}, kInt32);
        pick(0, (const float*)lg.device_ptr(), lg.numel(), (int32_t*)id.device_ptr_mut());
        int32_t got = -1;
        GTEN_HIP_OK(gten_hip_memcpy_d2h(&got, id.device_ptr(), sizeof(got)));
        return got;
    }

    void decode_set_tokens(int seq_i, const int32_t* ids, int first, int count)
    {
        ensure_decoder();
        GTEN_HIP_OK(gten_hip_decoder_set_tokens_seq(dec_, seq_i, ids, first, count));
    }
    // asynchronous: row n-1 of EVERY sequence
    void decode_step(int n, bool use_graph)
    {
        ensure_decoder();
        GTEN_HIP_OK(gten_hip_decoder_step(dec_, n, use_graph ? 1 : 0));
    }
    void decode_steps(int n_first, int count, bool use_graph)
    {
        ensure_decoder();
        GTEN_HIP_OK(gten_hip_decoder_steps(dec_, n_first, count, use_graph ? 1 : 0));
    }
    // greedy generation of every sequence with the sampler on the device (gten_hip_decoder_generate_multi): sequence q's
    // ids [0, n_first[q]) are set and its caches hold rows [0, n_first[q] - 1); out is [n_seq][max_new]
    // (max_new_seq: each sequence's own bound, may be null)
    void decode_generate(const int* n_first, int max_new, int eos, int32_t* out, int* n_out, const int* max_new_seq = nullptr)
    {
        ensure_decoder();
        GTEN_HIP_OK(gten_hip_decoder_generate_multi(dec_, n_first, max_new_seq, max_new, eos, out, n_out));
    }
    // the shared decoder itself, for what sets requests on it (host/generate.h, host/capi_bias.cpp, host/capi_logprobs.cpp)
    gten_hip_decoder* decoder_handle()
    {
        ensure_decoder();
        return dec_;
    }
    // asynchronous: row n[q]-1 of sequence q (continuous batching)
    void decode_step_ragged(const int* n_per_seq, bool use_graph)
    {
        ensure_decoder();
        GTEN_HIP_OK(gten_hip_decoder_step_ragged(dec_, n_per_seq, use_graph ? 1 : 0));
    }
    int decode_result(int seq_i, int n)
    {
        ensure_decoder();
        int32_t tok = -1;
        GTEN_HIP_OK(gten_hip_decoder_result_seq(dec_, seq_i, n, &tok));
        return tok;
    }
    void decode_logits(int seq_i, float* out)
    {
        ensure_decoder();
        GTEN_HIP_OK(gten_hip_decoder_logits_seq(dec_, seq_i, out));
    }
    // head-major K / V shadows of the shared decoder (gten_hip_decoder_kv_info)
    void kv_info(int* head_major, unsigned long long* seq_imports, unsigned long long* import_launches)
    {
        ensure_decoder();
        GTEN_HIP_OK(gten_hip_decoder_kv_info(dec_, head_major, seq_imports, import_launches));
    }
    double decode_time_family(int family, int n, int reps, int* launches)
    {
        ensure_decoder();
        double us = 0.0;
        // (a family this decoder's step does not launch is reported, not fatal: < 0)
        if (gten_hip_decoder_time_family(dec_, family, n, reps, &us, launches) != 0) return -1.0;
        return us;
    }

    // ---- continuous batching: a queue of prompts served through the n_seq slots.  The scheduler is ServeQueue (host/serve.h, where
    // the stats, sample groups and session items are explained; its decisions: host/serve_plan.h); `pick` chooses the ids
    // (host/generate.h, ServePolicy).
    struct ServeStats { int64_t prompt_tokens = 0, new_tokens = 0, steps = 0, admissions = 0, lane_steps = 0, moved = 0; int lane_rows = 0; double prefill_s = 0.0, decode_s = 0.0; };
    template <class Pick>
    ServeStats serve_with(const std::vector<std::vector<int32_t>>& prompts, int max_tokens, int eos, int slice,
                          std::vector<std::vector<int32_t>>* out, Each<int32_t> max_new, Each<int32_t> group_of, Pick& pick,
                          Each<int32_t> session = Each<int32_t>{nullptr, -1})
    {
        ServeQueue<Pick> queue(*this, prompts, max_tokens, eos, slice, out, max_new, group_of, pick, session);
        return queue.run();
    }

    // Cache sets beyond the sequences' own that serve() fills ahead (-1: a quarter of the slots, at most 64, for wide batches; 0:
    // a prompt is only processed once a slot is free, the behaviour before round 4)
    void set_serve_spares(int n) { serve_spares_ = n; }
    // Percent of the slots that get a processed prompt before a queue's first slice starts (wide batches; default 100)
    void set_serve_ramp(int percent) { serve_ramp_ = std::min(std::max(percent, 0), 100); }

    // Tests: k > 0 fixes the admission schedule -- exactly k prompts are processed beside every slice (as far as slots and
    // queue allow) instead of "as many as fit while the slice runs", so that a run is repeatable slice by slice.
    void set_serve_schedule(int k) { serve_schedule_ = k; }

    // ---- sample groups (include/gten_host_samples.h).  A prompt behind fewer rows than one full chunk of the decoder's shadows
    // (DEC_CHUNK) has nothing to read from a record.
    static constexpr int kGroupMinRows = 256;
    // group records a queue may hold at a time: -1: the default; 0: never take one (the members decode on their own copies); at most
    // kGroupsMax.  THE DEFAULT IS 0: measured (profiles/samples_cost.json), the records make the shared step 1 %
    // faster, but the queue's new tok/s with them lies inside the spread of the runs without -- the rule PFX_SHARED_DEFAULT was
    // decided by leaves them off.
    static constexpr int kGroupsCapDefault = 0;
    void set_groups_cap(int cap) { groups_cap_ = cap < 0 ? -1 : std::min(cap, kGroupsMax); }
    // items that were copies of another item's prompt pass, the prompt rows not computed for them, the groups that got a record
    // and those that did not (all since this batch was made), the records in use now
    // the group records of the shared decoder, for callers that drive the steps themselves (tests): gten_hip_decoder_group_set with
    // the caches of cache set c (c < 0: release), gten_hip_decoder_group_share, return codes and all; 0 without the entry points
    int group_set_rc(int g, int c, int rows)
    {
        if (!detail::groups_decode().set) return 0;
        ensure_decoder();
        return detail::groups_decode().set(dec_, g, c >= 0 ? set_kv(c) : nullptr, c >= 0 ? rows : 0);
    }
    int group_share_rc(int seq_i, int g, int rows)
    {
        if (!detail::groups_decode().share) return 0;
        ensure_decoder();
        return detail::groups_decode().share(dec_, seq_i, g, rows);
    }
    // gten_hip_decoder_groups_info on the shared decoder (-1 / 0 without the entry points)
    void groups_decode_info(int seq_i, int g, int* seq_group, int* seq_chunks, int* rows, unsigned long long* imports, int* sharers)
    {
        if (seq_group) *seq_group = -1;
        if (seq_chunks) *seq_chunks = 0;
        if (rows) *rows = 0;
        if (imports) *imports = 0;
        if (sharers) *sharers = 0;
        if (!detail::groups_decode().info) return;
        ensure_decoder();
        GTEN_HIP_OK(detail::groups_decode().info(dec_, seq_i, g, seq_group, seq_chunks, rows, imports, sharers));
    }
    void samples_info(unsigned long long* copies, unsigned long long* rows_saved, unsigned long long* recorded, unsigned long long* unrecorded, int* records_now) const
    {
        if (copies) *copies = samples_copies_;
        if (rows_saved) *rows_saved = samples_rows_saved_;
        if (recorded) *recorded = groups_recorded_;
        if (unrecorded) *unrecorded = groups_unrecorded_;
        if (records_now) *records_now = group_records_now_;
    }

private:
    unsigned long long samples_copies_ = 0, samples_rows_saved_ = 0, groups_recorded_ = 0, groups_unrecorded_ = 0;
    int group_records_now_ = 0;
    int groups_cap_ = -1;
    std::vector<std::unique_ptr<TinyLlama>> seqs_;
    std::vector<std::unique_ptr<TinyLlama>> spares_;   // spare cache sets of serve()
    std::vector<std::vector<gten_hip_kv_ptrs>> set_kv_;      // per cache set: its layers' cache pointers (gten_hip_decoder_slot_bind)
    std::unique_ptr<TinyLlama> pre_;         // the shared row matrix of batched prompt processing (prefill_many), made on first use
    struct Prefix {
        std::unique_ptr<TinyLlama> set;      // the cache set that holds this prefix's K / V rows (set_prefix_at)
        std::vector<int32_t> ids;            // the prefix (empty: none registered at this index)
        unsigned long long prompts_shared = 0;   // prompts that took the short way behind it
        unsigned long long rows_computed = 0;    // ... and the rows computed for them
    } pfx_[kPrefixesMax];
    struct Session {
        bool open = false;
        std::unique_ptr<TinyLlama> set;      // its own cache set (made on first open, kept for the next session at this index)
        std::vector<int32_t> ids;            // the history
        int rows = 0;                        // leading positions with valid K / V rows
    };
    std::vector<Session> sessions_;
    unsigned long long sess_turns_ = 0, sess_turns_continued_ = 0, sess_rows_computed_ = 0, sess_rows_kept_ = 0;
    unsigned long long turns_continued_ = 0, rows_extended_ = 0, rows_kept_ = 0, rows_computed_one_ = 0;    // extend_many (extend_info)
    unsigned long long rows_computed_ = 0;   // prompt rows computed in segmented calls (the prefix's own rows not counted)
    std::unique_ptr<Tensor> first_ids_;      // [kPreMax] int32 on the device: the prompts' first ids (gten_hip_argmax_row)
    gten_hip_decoder* dec_ = nullptr;
    int n_ctx_;
    ModuleDtype dtype_;
    TinyLLamaParams params_;
    int serve_schedule_ = 0;
    int serve_spares_ = -1;
    int serve_ramp_ = 100;
    std::vector<int> set_share_;             // per cache set: its rows [0, P) are a copy of a prefix set's (0: no such mark)
    std::vector<int> set_which_;             // ... of which prefix (where the mark is not 0)
    bool in_serve_ = false;                  // serve() is running: sets are bound to slots by the scheduler

    int& share_mark(int c)
    {
        if ((int)set_share_.size() < index_space()) set_share_.resize((size_t)index_space(), 0);
        return set_share_[(size_t)c];
    }
    int& which_mark(int c)
    {
        if ((int)set_which_.size() < index_space()) set_which_.resize((size_t)index_space(), 0);
        return set_which_[(size_t)c];
    }
    // every mark that speaks of prefix w is void
    void forget_prefix_marks(int w)
    {
        for (size_t c = 0; c < set_share_.size(); c++)
            if (set_share_[c] > 0 && which_mark((int)c) == w) set_share_[c] = 0;
    }
    // the decoder's entry points: those of several prefixes where installed, else those of one prefix for index 0
    int decoder_share(int q, int w, int rows)
    {
        if (detail::prefixes_decode().share) return detail::prefixes_decode().share(dec_, q, w, rows);
        if (w == 0 && detail::prefix_decode().slot_share) return detail::prefix_decode().slot_share(dec_, q, rows);
        return 0;
    }
    // prefix w's set's caches to the shared decoder (on) or "no prefix at index w" (off): either way every slot that shares w is
    // taken off the shared copy first and every mark that speaks of w is void -- they spoke of the previous prefix
    void decoder_prefix(int w, bool on)
    {
        forget_prefix_marks(w);
        if (!dec_) return;
        const gten_hip_kv_ptrs* kvp = nullptr;
        std::vector<gten_hip_kv_ptrs> kv;
        int len = 0;
        if (on && !pfx_[w].ids.empty() && pfx_[w].set) {
            gten_hip_decoder_desc di;
            std::vector<gten_hip_layer_ptrs> Li;
            pfx_[w].set->describe(&di, &Li);
            for (auto& p : Li) kv.push_back(gten_hip_kv_ptrs{p.kcache, p.vcache});
            kvp = kv.data();
            len = (int)pfx_[w].ids.size();
        }
        if (detail::prefixes_decode().set) GTEN_HIP_OK(detail::prefixes_decode().set(dec_, w, kvp, len));
        else if (w == 0 && detail::prefix_decode().prefix_set) GTEN_HIP_OK(detail::prefix_decode().prefix_set(dec_, kvp, len));
    }

    const gten_hip_kv_ptrs* set_kv(int c)
    {
        if ((int)set_kv_.size() < index_space()) set_kv_.resize((size_t)index_space());
        std::vector<gten_hip_kv_ptrs>& kv = set_kv_[(size_t)c];
        if (kv.empty()) {
            gten_hip_decoder_desc di;
            std::vector<gten_hip_layer_ptrs> Li;
            cset(c).describe(&di, &Li);
            for (auto& p : Li) kv.push_back(gten_hip_kv_ptrs{p.kcache, p.vcache});
        }
        return kv.data();
    }

    void ensure_decoder()
    {
        if (dec_) return;
        gten_hip_decoder_desc d;
        std::vector<gten_hip_layer_ptrs> L, Li;
        seqs_[0]->describe(&d, &L);
        std::vector<gten_hip_kv_ptrs> kv;
        for (auto& m : seqs_) {
            gten_hip_decoder_desc di;
            m->describe(&di, &Li);
            for (auto& p : Li) kv.push_back(gten_hip_kv_ptrs{p.kcache, p.vcache});
        }
        GTEN_HIP_OK(gten_hip_decoder_create_multi(&d, L.data(), kv.data(), (int)seqs_.size(), &dec_));
        for (int w = 0; w < kPrefixesMax; w++)
            if (!pfx_[w].ids.empty()) decoder_prefix(w, true);     // (a prefix set before the decoder existed)
    }
};

// Greedy loop of tinyllama.cpp:395-440 on token ids (no tokenizer): iteration 0
// is the prefill (start_pos 0), later iterations compute one row; argmax with
// strict '>' so the first maximum wins; stop at `eos`.
inline int greedy_sample(TinyLlama& model, std::vector<int32_t>& tokens, const int n_predict, const int eos)
{
    const int max_iters = n_predict - (int)tokens.size();
    for (int i = 0; i < max_iters; i++) {
        Tensor input{tokens.data(), {(int)tokens.size()}, kInt32};
        const int start_pos = (i == 0) ? 0 : input.numel() - 1;
        Tensor logits = model.logits(input, start_pos);
        Timer sample_timer{&model.sample_time};
        const int n = logits.numel();
        const float* p = const_cast<const Tensor&>(logits).data_ptr<float>();
        float best = -std::numeric_limits<float>::infinity();
        int best_i = 0;
        for (int j = 0; j < n; j++)
            if (p[j] > best) { best = p[j]; best_i = j; }
        if (best_i == eos) break;
        tokens.push_back(best_i);
    }
    return (int)tokens.size();
}

} // namespace gten

#include "serve.h"                       // ServeQueue, which serve_with instantiates
