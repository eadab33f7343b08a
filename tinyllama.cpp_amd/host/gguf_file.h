// gguf_file.h -- a llama-family GGUF file (version 2 or 3, little-endian) read for the command line's --from-gguf: the header, the
// key / value section (all 13 value types; only llama.block_count, llama.attention.head_count, head_count_kv and general.alignment
// are kept), the tensor infos, and each tensor's bytes handed to QuantLoader::set_weight_from_gguf as they lie in the file
// (include/gten_host_gguf.h).  Device-free up to that call.  tinyllama.cpp_amd/convert.py's open_gguf is the
// same reader in Python; what cannot be loaded is refused by name through GTEN_ASSERTM.
#pragma once

#include <cstdint>
#include <fstream>
#include <map>
#include <string>
#include <vector>

#include "quant_load.h"

namespace gten {

class GgufFile {
public:
    struct Info { int type; std::vector<uint64_t> ne; uint64_t offset; };

    explicit GgufFile(std::ifstream& f) : f_{f}
    {
        char magic[4] = {};
        f_.read(magic, 4);
        GTEN_ASSERTM(f_.good() && std::string(magic, 4) == "GGUF", "Not a GGUF file (bad magic).");
        const uint32_t version = get<uint32_t>();
        GTEN_ASSERTM((version & 0xFFFFu) != 0 || version == 0, "A big-endian GGUF file: only little-endian files are read.");
        GTEN_ASSERTM(version == 2 || version == 3, "GGUF version %u is not supported (2 or 3).", version);
        const uint64_t n_tensors = get<uint64_t>(), n_kv = get<uint64_t>();
        for (uint64_t i = 0; i < n_kv; i++) {
            const std::string key = str();
            const uint32_t vt = get<uint32_t>();
            const bool keep = key == "llama.block_count" || key == "llama.attention.head_count" || key == "llama.attention.head_count_kv" ||
                              key == "general.alignment";
            const int64_t v = value(vt);
            if (keep && vt != 8 && vt != 9) kv_[key] = v;
        }
        alignment_ = kv_.count("general.alignment") ? (uint64_t)kv_["general.alignment"] : 32;
        GTEN_ASSERTM(alignment_ > 0, "GGUF: general.alignment is 0.");
        for (uint64_t i = 0; i < n_tensors; i++) {
            const std::string name = str();
            Info info;
            const uint32_t n_dims = get<uint32_t>();
            GTEN_ASSERTM(n_dims >= 1 && n_dims <= 4, "GGUF tensor `%s` has %u dimensions.", name.c_str(), n_dims);
            for (uint32_t d = 0; d < n_dims; d++) info.ne.push_back(get<uint64_t>());
            info.type = (int)get<uint32_t>();
            info.offset = get<uint64_t>();
            infos_[name] = info;
        }
        data0_ = ((uint64_t)f_.tellg() + alignment_ - 1) / alignment_ * alignment_;
    }

    int64_t key(const char* k, int64_t otherwise = -1) const { return kv_.count(k) ? kv_.at(k) : otherwise; }

    // every weight of `model` from its tensor: token_embd, blk.N.*, output_norm, output (token_embd again when the file has none)
    void load_into(TinyLlama& model, QuantLoader& quant)
    {
        Timer load_timer{&model.load_time};
        const int n_layers = (model.n_weights() - 3) / 9;
        const int64_t n_head = key("llama.attention.head_count"), n_head_kv = key("llama.attention.head_count_kv", n_head);
        GTEN_ASSERTM(key("llama.block_count") == n_layers, "The GGUF file has %lld blocks, the model %d.", (long long)key("llama.block_count"), n_layers);
        GTEN_ASSERTM(n_head > 0 && n_head_kv > 0, "The GGUF file lacks llama.attention.head_count.");
        static const char* block[9] = {"attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down", "attn_norm", "ffn_norm"};
        std::vector<char> payload;
        for (int idx = 0; idx < model.n_weights(); idx++) {
            std::string name = idx == 0 ? "token_embd.weight" : idx == model.n_weights() - 2 ? "output_norm.weight" : idx == model.n_weights() - 1 ? "output.weight"
                               : "blk." + std::to_string((idx - 1) / 9) + "." + block[(idx - 1) % 9] + ".weight";
            if (name == "output.weight" && !infos_.count(name)) name = "token_embd.weight";
            GTEN_ASSERTM(infos_.count(name), "The GGUF tensor `%s` is missing.", name.c_str());
            const Info& t = infos_.at(name);
            const Tensor& w = model.weight(idx);
            const uint64_t rows = w.is_2d() ? (uint64_t)w.dimsize(0) : 1, cols = (uint64_t)w.dimsize(w.ndims() - 1);
            GTEN_ASSERTM(t.ne[0] == cols && (t.ne.size() > 1 ? t.ne[1] : 1) == rows && t.ne.size() <= 2,
                         "The GGUF tensor `%s` has the wrong shape: the model's is %llu x %llu.", name.c_str(), (unsigned long long)rows, (unsigned long long)cols);
            const bool dense = t.type == 0 || t.type == 1 || t.type == 30;
            const size_t nbytes = dense ? rows * cols * (t.type == 0 ? 4 : 2) : gten_hip_gguf_src_bytes(t.type, (int)rows, (int)cols);
            GTEN_ASSERTM(nbytes, "The GGUF tensor `%s` has ggml type %d, which is not supported for %llu columns (F32 0, F16 1, BF16 30, Q4_0 2, Q5_0 6, Q8_0 8, Q4_K 12, Q5_K 13, Q6_K 14).",
                         name.c_str(), t.type, (unsigned long long)cols);
            GTEN_ASSERTM(t.offset % alignment_ == 0, "The GGUF tensor `%s` lies off the file's alignment.", name.c_str());
            payload.resize(nbytes);
            f_.clear();
            f_.seekg((std::streamoff)(data0_ + t.offset));
            f_.read(payload.data(), (std::streamsize)nbytes);
            GTEN_ASSERTM(f_.good(), "The GGUF file ends inside tensor `%s`.", name.c_str());
            int n_map = (idx - 1) % 9 == 0 && idx > 0 && idx < model.n_weights() - 2 ? (int)n_head : (idx - 1) % 9 == 1 && idx > 0 && idx < model.n_weights() - 2 ? (int)n_head_kv : 0;
            if (dense && n_map) {                                   // a dense q / k: the rows back into order here, nothing to decode
                const size_t rb = nbytes / rows, D = rows / (size_t)n_map;
                std::vector<char> ordered(nbytes);
                for (size_t r = 0; r < rows; r++) {
                    const size_t h = r / D, rem = r % D, src = h * D + 2 * (rem % (D / 2)) + rem / (D / 2);
                    std::copy(payload.begin() + (long)(src * rb), payload.begin() + (long)((src + 1) * rb), ordered.begin() + (long)(r * rb));
                }
                payload.swap(ordered);
                n_map = 0;
            }
            const int rc = quant.set_weight_from_gguf(model, idx, payload.data(), nbytes, t.type, n_map);
            GTEN_ASSERTM(rc == 0, "The GGUF tensor `%s` (ggml type %d) could not be loaded on the device (rc %d): %s", name.c_str(), t.type, rc,
                         rc == -3 ? "the type is not supported for this tensor" : gten_hip_last_error());
        }
        quant.release();
    }

private:
    template <typename T> T get()
    {
        T v{};
        f_.read(reinterpret_cast<char*>(&v), sizeof(T));
        GTEN_ASSERTM(f_.good(), "The GGUF file ends inside its header.");
        return v;
    }
    std::string str()
    {
        const uint64_t n = get<uint64_t>();
        GTEN_ASSERTM(n < (1u << 24), "Corrupt string in the GGUF header.");
        std::string s((size_t)n, '\0');
        f_.read(s.data(), (std::streamsize)n);
        GTEN_ASSERTM(f_.good(), "The GGUF file ends inside its header.");
        return s;
    }
    // one value of type vt, consumed; integers and bool come back, everything else as 0
    int64_t value(uint32_t vt)
    {
        switch (vt) {
        case 0: return get<uint8_t>();
        case 1: return get<int8_t>();
        case 2: return get<uint16_t>();
        case 3: return get<int16_t>();
        case 4: return get<uint32_t>();
        case 5: return get<int32_t>();
        case 6: get<float>(); return 0;
        case 7: return get<uint8_t>();
        case 8: str(); return 0;
        case 9: {
            const uint32_t et = get<uint32_t>();
            const uint64_t n = get<uint64_t>();
            for (uint64_t i = 0; i < n; i++) value(et);
            return 0;
        }
        case 10: return (int64_t)get<uint64_t>();
        case 11: return get<int64_t>();
        case 12: get<double>(); return 0;
        default: GTEN_ASSERTM(false, "GGUF key / value type %u is not a GGUF value type.", vt); return 0;
        }
    }

    std::ifstream& f_;
    std::map<std::string, int64_t> kv_;
    std::map<std::string, Info> infos_;
    uint64_t alignment_ = 32, data0_ = 0;
};

} // namespace gten
