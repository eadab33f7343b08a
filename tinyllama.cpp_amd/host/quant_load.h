// quant_load.h -- weights from UNQUANTISED bytes (include/gten_host_quant.h): a tensor's elements go up in the dtype they
// have (f32 / bf16 / f16) into one staging buffer in HBM, grown on demand, and gten_hip_quantize_weight writes the model's
// weight tensor from there -- Q8 / Q4 quantised and packed, f16 rounded; norm vectors (always f16) take the same way.
// set_weight_from_lora merges a LoRA adapter on the way (include/gten_hip_lora.h); set_weight_from_search writes
// Q4 through the importance-weighted delta search (include/gten_hip_calib.h).
// set_weight_from_gguf takes a GGUF tensor's ggml block stream, decoded on the device (include/gten_hip_gguf.h).
// set_weight_from_w4 takes the four tensors of a GPTQ / AWQ linear, transposed on the device (include/gten_hip_w4.h).
// The one host header that names include/gten_hip_quant.h, include/gten_hip_lora.h, include/gten_hip_gguf.h and include/gten_hip_w4.h
// beside gten/tensor.h.
#pragma once

#include <fstream>
#include <string>
#include <vector>

#include "../../include/gten_hip_gguf.h"
#include "../../include/gten_hip_lora.h"
#include "../../include/gten_hip_quant.h"
#include "../../include/gten_hip_w4.h"
#include "tinyllama_model.h"

namespace gten {

class QuantLoader {
public:
    QuantLoader() = default;
    QuantLoader(const QuantLoader&) = delete;
    QuantLoader& operator=(const QuantLoader&) = delete;
    ~QuantLoader() { release(); }

    // bytes weight idx takes in a source dtype (0: bad index or code)
    static size_t src_bytes(TinyLlama& model, int idx, int src_dtype)
    {
        if (idx < 0 || idx >= model.n_weights()) return 0;
        const Tensor& w = model.weight(idx);
        return gten_hip_quant_src_bytes(src_dtype, w.is_2d() ? w.dimsize(0) : 1, w.dimsize(w.ndims() - 1));
    }

    // 0; -1 bad index or source dtype; -2 nbytes is not the tensor's size in that dtype; else the device library's code
    // (gten_hip_last_error() has the text: a NaN or an infinity among the elements is one)
    int set_weight_from(TinyLlama& model, int idx, const void* bytes, size_t nbytes, int src_dtype)
    {
        const size_t need = src_bytes(model, idx, src_dtype);
        if (!need || !bytes) return -1;
        if (nbytes != need) return -2;
        if (const int rc = stage_source(bytes, nbytes)) return rc;
        return model.weight(idx).device_weight_from(stage_, src_dtype);
    }

    // The same with a LoRA adapter merged in on the device (include/gten_host_lora.h): a [rank][cols] and b [rows][rank] in
    // ab_dtype go up beside the source, into a second buffer of their own.  Only the seven linear weights of a block take
    // one: -3 for embed_tokens, lm_head and the norm vectors (lora_error() names which); -1 also for a bad rank or ab_dtype.
    int set_weight_from_lora(TinyLlama& model, int idx, const void* bytes, size_t nbytes, int src_dtype, const void* a, const void* b,
                             int rank, int ab_dtype, float scale)
    {
        const size_t need = src_bytes(model, idx, src_dtype);
        if (!need || !bytes || !a || !b || rank < 1 || rank > GTEN_HIP_LORA_MAX_RANK) return -1;
        if (nbytes != need) return -2;
        const int last = model.n_weights() - 1;
        if (idx == 0 || idx >= last - 1 || (idx - 1) % 9 >= 7) {
            lora_error_ = std::string("set_weight_from_lora: weight ") + std::to_string(idx) + " is " +
                          (idx == 0 ? "embed_tokens" : idx == last ? "lm_head" : "a norm vector") +
                          ": only q, k, v, o, gate, up and down of a block take an adapter";
            return -3;
        }
        const Tensor& w = model.weight(idx);
        const size_t a_bytes = gten_hip_quant_src_bytes(ab_dtype, rank, w.dimsize(1)), b_bytes = gten_hip_quant_src_bytes(ab_dtype, w.dimsize(0), rank);
        if (!a_bytes || !b_bytes) return -1;
        const size_t b_at = (a_bytes + 15) & ~(size_t)15;            // B starts 16-byte aligned behind A
        if (b_at + b_bytes > ab_cap_) {
            if (ab_) gten_hip_free(ab_);
            ab_ = nullptr;
            ab_cap_ = 0;
            detail::ensure_runtime();
            if (const int rc = gten_hip_malloc(&ab_, b_at + b_bytes)) return rc;
            ab_cap_ = b_at + b_bytes;
        }
        if (const int rc = stage_source(bytes, nbytes)) return rc;
        if (const int rc = gten_hip_memcpy_h2d(ab_, a, a_bytes)) return rc;
        if (const int rc = gten_hip_memcpy_h2d((char*)ab_ + b_at, b, b_bytes)) return rc;
        return model.weight(idx).device_weight_from(stage_, src_dtype, ab_, (const char*)ab_ + b_at, rank, ab_dtype, scale);
    }
    const char* lora_error() const { return lora_error_.c_str(); }

    // A block linear of a Q4 model through the device's delta search (include/gten_host_calib.h, which checks what it takes):
    // importance f32 [cols] goes up beside the source, into the second buffer; null: every weight 1
    int set_weight_from_search(TinyLlama& model, int idx, const void* bytes, size_t nbytes, int src_dtype, const float* importance)
    {
        const size_t need = src_bytes(model, idx, src_dtype);
        if (!need || !bytes) return -1;
        if (nbytes != need) return -2;
        Tensor& w = model.weight(idx);
        const size_t imp_bytes = (size_t)w.dimsize(1) * sizeof(float);
        if (importance && imp_bytes > ab_cap_) {
            if (ab_) gten_hip_free(ab_);
            ab_ = nullptr;
            ab_cap_ = 0;
            detail::ensure_runtime();
            if (const int rc = gten_hip_malloc(&ab_, imp_bytes)) return rc;
            ab_cap_ = imp_bytes;
        }
        if (const int rc = stage_source(bytes, nbytes)) return rc;
        if (importance)
            if (const int rc = gten_hip_memcpy_h2d(ab_, importance, imp_bytes)) return rc;
        return w.device_weight_search(stage_, src_dtype, importance ? (const float*)ab_ : nullptr);
    }

    // Weight idx from the bytes of a GGUF tensor of ggml type `ggml_type` (include/gten_host_gguf.h).  A block format: the block
    // stream goes up as it lies in the file and include/gten_hip_gguf.h decodes it, row-mapped by n_head, while it quantises.  The
    // dense types (F32 0, F16 1, BF16 30 -- every norm vector) take set_weight_from.  -3: a code that is neither, a block format for
    // a norm vector, a dense type with a row map.
    int set_weight_from_gguf(TinyLlama& model, int idx, const void* bytes, size_t nbytes, int ggml_type, int n_head)
    {
        if (idx < 0 || idx >= model.n_weights() || !bytes || n_head < 0) return -1;
        if (ggml_type == 0 || ggml_type == 1 || ggml_type == 30) {
            if (n_head != 0) return -3;
            return set_weight_from(model, idx, bytes, nbytes, ggml_type == 0 ? GTEN_HIP_SRC_F32 : ggml_type == 1 ? GTEN_HIP_SRC_F16 : GTEN_HIP_SRC_BF16);
        }
        Tensor& w = model.weight(idx);
        if (!w.is_2d()) return -3;
        const size_t need = gten_hip_gguf_src_bytes(ggml_type, w.dimsize(0), w.dimsize(1));
        if (!need) return gten_hip_gguf_src_bytes(ggml_type, 1, 256) ? -2 : -3;      // the shape does not fit the format | not a format
        if (nbytes != need) return -2;
        if (const int rc = stage_source(bytes, nbytes)) return rc;
        return w.device_weight_from_gguf(stage_, ggml_type, n_head);
    }

    // A block linear from the qweight / qzeros / scales (/ g_idx) of its GPTQ or AWQ layer (include/gten_host_w4.h): the pieces go up
    // behind each other, each from a 16-byte boundary, and include/gten_hip_w4.h unpacks, transposes and quantises them in one launch.
    // -2: a shape or group_size the layout cannot hold; -3: embed_tokens, lm_head and the norm vectors, dense in these checkpoints.
    int set_weight_from_w4(TinyLlama& model, int idx, const void* qweight, const void* qzeros, const void* scales, const void* g_idx, int layout,
                           int zero_offset, int group_size)
    {
        if (idx < 0 || idx >= model.n_weights() || !qweight || !qzeros || !scales) return -1;
        if (idx == 0 || idx >= model.n_weights() - 2 || (idx - 1) % 9 >= 7) return -3;
        Tensor& w = model.weight(idx);
        const void* piece[4] = {qweight, qzeros, scales, g_idx};
        size_t bytes[4], at[4], total = 0;
        for (int i = 0; i < 4; i++) {
            bytes[i] = piece[i] ? gten_hip_w4_src_bytes(layout, i, w.dimsize(0), w.dimsize(1), group_size) : 0;
            if (piece[i] && !bytes[i]) return i == 3 ? -1 : -2;       // (a g_idx for AWQ is a bad argument, not a bad shape)
            at[i] = total;
            total += (bytes[i] + 15) & ~(size_t)15;
        }
        if (const int rc = stage_reserve(total)) return rc;
        for (int i = 0; i < 4; i++)
            if (piece[i])
                if (const int rc = gten_hip_memcpy_h2d((char*)stage_ + at[i], piece[i], bytes[i])) return rc;
        return w.device_weight_from_w4(stage_, (char*)stage_ + at[1], (char*)stage_ + at[2], g_idx ? (char*)stage_ + at[3] : nullptr, layout, zero_offset,
                                       group_size);
    }

    // An f16 .gten file into a model of ANY weight dtype: TinyLlama::load_from_ckpt's framing and messages, each payload
    // checked against the tensor's f16 size and handed to set_weight_from.  An f16 model reads the file as it always did.
    void load_gten_f16(TinyLlama& model, std::ifstream& ckpt)
    {
        if (model.weight(0).dtype() == kFloat16) {
            model.load_from_ckpt(ckpt);
            return;
        }
        Timer load_timer{&model.load_time};
        int64_t magic = 0;
        ckpt.read(reinterpret_cast<char*>(&magic), sizeof(magic));
        GTEN_ASSERTM(magic == 0x454c49464e455447LL, "Magic number in the binary does not match the expected one.");
        std::vector<char> payload;
        for (int i = 0; i < model.n_weights(); i++) {
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
            const size_t want = src_bytes(model, i, GTEN_HIP_SRC_F16);
            GTEN_ASSERTM(static_cast<size_t>(nbytes) == want, "Weight `%s` data size: %d does not match the expected size: %zu.",
                         name.c_str(), nbytes, want);
            payload.resize(want);
            ckpt.read(payload.data(), nbytes);
            GTEN_ASSERTM(ckpt.good(), "Checkpoint ended inside weight `%s`.", name.c_str());
            const int rc = set_weight_from(model, i, payload.data(), want, GTEN_HIP_SRC_F16);
            GTEN_ASSERTM(rc == 0, "Weight `%s` could not be quantised on the device: %s", name.c_str(), gten_hip_last_error());
        }
        release();
    }

    void release()
    {
        if (stage_) gten_hip_free(stage_);
        if (ab_) gten_hip_free(ab_);
        stage_ = ab_ = nullptr;
        cap_ = ab_cap_ = 0;
    }

private:
    // the staging buffer, grown on demand
    int stage_reserve(size_t nbytes)
    {
        if (nbytes > cap_) {
            if (stage_) gten_hip_free(stage_);
            stage_ = nullptr;
            cap_ = 0;
            detail::ensure_runtime();
            if (const int rc = gten_hip_malloc(&stage_, nbytes)) return rc;
            cap_ = nbytes;
        }
        return 0;
    }
    // the source bytes into it
    int stage_source(const void* bytes, size_t nbytes)
    {
        if (const int rc = stage_reserve(nbytes)) return rc;
        return gten_hip_memcpy_h2d(stage_, bytes, nbytes);
    }

    void* ab_ = nullptr;        // HBM, one adapter's A, then B from the next 16-byte boundary
    size_t ab_cap_ = 0;
    std::string lora_error_;
    void* stage_ = nullptr;     // HBM, source-dtype bytes of one tensor
    size_t cap_ = 0;
};

} // namespace gten
