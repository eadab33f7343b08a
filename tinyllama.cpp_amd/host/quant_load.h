// quant_load.h -- weights from UNQUANTISED bytes (include/gten_host_quant.h): a tensor's elements go up in the dtype they
// have (f32 / bf16 / f16) into one staging buffer in HBM, grown on demand, and gten_hip_quantize_weight writes the model's
// weight tensor from there -- Q8 / Q4 quantised and packed, f16 rounded; norm vectors (always f16) take the same way.
// The one host header that names include/gten_hip_quant.h beside gten/tensor.h.
#pragma once

#include <fstream>
#include <string>
#include <vector>

#include "../../include/gten_hip_quant.h"
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
        if (need > cap_) {
            release();
            detail::ensure_runtime();
            if (const int rc = gten_hip_malloc(&stage_, need)) return rc;
            cap_ = need;
        }
        if (const int rc = gten_hip_memcpy_h2d(stage_, bytes, nbytes)) return rc;
        return model.weight(idx).device_weight_from(stage_, src_dtype);
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
        stage_ = nullptr;
        cap_ = 0;
    }

private:
    void* stage_ = nullptr;     // HBM, source-dtype bytes of one tensor
    size_t cap_ = 0;
};

} // namespace gten
