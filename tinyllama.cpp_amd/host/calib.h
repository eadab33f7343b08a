// calib.h -- the state behind include/gten_host_calib.h: per-layer f64 accumulators in HBM for the energy of the four tensors that
// feed a block's linears, filled by gten_hip_calib_col_energy from the rows a prompt pass has just computed (host/capi_calib.cpp
// installs the hook of gten/modules.h and links the entry point; nothing here names it, so code built on capi_handles.h alone does
// not need the symbol).  DESIGN.md 3.28.
#pragma once

#include <string>
#include <vector>

#include "tinyllama_model.h"

namespace gten {

struct Calib {
    // [layer][which]: which 0 the input of q | k | v, 1 of o, 2 of gate | up (n_embd wide), 3 of down (n_ffn wide)
    std::vector<void*> acc;
    TinyLlama* model = nullptr;          // whose blocks collect
    int n_layers = 0, n_embd = 0, n_ffn = 0;
    long long rows = -1;                 // rows layer 0 has seen since begin; -1: never begun
    bool collecting = false;
    int rc = 0;                          // the first device error of a collection (the hook cannot return one)
    std::string error;                   // the text of the last -3 of set_weight_from

    Calib() = default;
    Calib(const Calib&) = delete;
    Calib& operator=(const Calib&) = delete;
    ~Calib()
    {
        stop();
        release();
    }

    // collection off: the hook of gten/modules.h is taken down if it is this object's
    void stop()
    {
        detail::CalibRows& hook = detail::calib_rows();
        if (hook.owner == this) hook = detail::CalibRows{};
        collecting = false;
    }

    int width(int which) const { return which == 3 ? n_ffn : n_embd; }
    double* at(int layer, int which) const { return static_cast<double*>(acc[(size_t)layer * 4 + which]); }

    // zeroed accumulators for a model of these sizes
    int reset(int layers, int embd, int ffn)
    {
        release();
        n_layers = layers; n_embd = embd; n_ffn = ffn;
        acc.assign((size_t)layers * 4, nullptr);
        for (int i = 0; i < layers * 4; i++) {
            const size_t bytes = (size_t)width(i % 4) * sizeof(double);
            if (const int e = gten_hip_malloc(&acc[(size_t)i], bytes)) return e;
            if (const int e = gten_hip_memset(acc[(size_t)i], 0, bytes)) return e;
        }
        rows = 0;
        rc = 0;
        return 0;
    }

    void release()
    {
        for (void* p : acc)
            if (p) gten_hip_free(p);
        acc.clear();
        rows = -1;
    }

    // the layer of a block of `model` or of its segmented-prompt model (score_many's texts of 16+ ids run there); -1: neither's
    static int layer_of(TinyLlama& model, const AttentionBlock& block, int n_layers)
    {
        for (int l = 0; l < n_layers; l++)
            if (&model.block(l) == &block) return l;
        if (TinyLlama* seg = model.segment_model_if())
            for (int l = 0; l < n_layers; l++)
                if (&seg->block(l) == &block) return l;
        return -1;
    }
};

} // namespace gten
