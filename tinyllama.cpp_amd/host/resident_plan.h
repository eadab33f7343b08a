// resident_plan.h -- which W.x launches of a single-sequence decode step load their weights with the DEFAULT cache policy, so that
// they stay in the memory-side cache from token to token, and which keep the nontemporal stream.  Device-free like
// serve_plan.h and beam_plan.h: the standard library only; the decoder computes the plan once at creation from its own layer table
// (csrc/gten_decode.hip), tests/host_resident_plan.cpp runs it on the CPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

namespace gten {

enum { kResidentQkv = 0, kResidentO = 1, kResidentGateUp = 2, kResidentDown = 3, kResidentHead = 4 };

// bytes of one 32-element weight block, deltas included: the device library's packed layouts
constexpr int kResidentBlockF16 = 64, kResidentBlockQ8 = 34, kResidentBlockQ4 = 18;

// one W.x launch of the step
struct ResidentLaunch {
    int family = 0;           // kResident*
    int layer = 0;            // (lm_head: the layer count)
    long long bytes = 0;      // the weight bytes the launch reads, deltas included
};

struct ResidentPlan {
    std::vector<char> resident;   // one entry per launch, in step order: 1 = default policy
    int launches = 0;             // how many are
    long long bytes = 0;          // their weight bytes
};

inline long long resident_weight_bytes(long long rows, long long cols, int block_bytes) { return rows * (cols / 32) * block_bytes; }

// the W.x launches of one step of a llama model in step order: per layer q|k|v, o, gate|up, down; then lm_head
inline std::vector<ResidentLaunch> resident_step_launches(int n_layers, int n_embd, int n_ffn, int kv_width, int n_vocab, int block_bytes)
{
    std::vector<ResidentLaunch> v;
    const long long E = n_embd, F = n_ffn, KV = kv_width;
    for (int l = 0; l < n_layers; l++) {
        v.push_back(ResidentLaunch{kResidentQkv, l, resident_weight_bytes(E + 2 * KV, E, block_bytes)});
        v.push_back(ResidentLaunch{kResidentO, l, resident_weight_bytes(E, E, block_bytes)});
        v.push_back(ResidentLaunch{kResidentGateUp, l, resident_weight_bytes(2 * F, E, block_bytes)});
        v.push_back(ResidentLaunch{kResidentDown, l, resident_weight_bytes(E, F, block_bytes)});
    }
    v.push_back(ResidentLaunch{kResidentHead, n_layers, resident_weight_bytes(n_vocab, E, block_bytes)});
    return v;
}

// The plan: launches in ascending order of their weight bytes (the first-byte latency is paid once per launch whatever the launch
// moves, so residency is worth most per byte on the smallest matrices), ties in step order; a launch is resident whole or not at all
// (it ends with its slowest row); launches are taken while the running sum stays within the budget and the FIRST one that does not
// fit ends the selection -- nothing smaller is squeezed in behind it, so the plan is monotone in the budget.
inline ResidentPlan resident_plan(const std::vector<ResidentLaunch>& step, long long budget)
{
    ResidentPlan p;
    p.resident.assign(step.size(), 0);
    std::vector<size_t> order(step.size());
    for (size_t i = 0; i < order.size(); i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return step[a].bytes < step[b].bytes; });
    for (size_t i : order) {
        const long long b = step[i].bytes;
        if (b < 0 || budget - p.bytes < b) break;
        p.resident[i] = 1;
        p.launches++;
        p.bytes += b;
    }
    return p;
}

// what is left of a setting of `all` bytes for the weights once the decoder's other default-policy traffic is taken off: its K / V
// rows at max_ctx and its activation scratch.  Never negative.
inline long long resident_budget(long long all, long long kv_bytes, long long scratch_bytes)
{
    return std::max(0ll, all - std::max(0ll, kv_bytes) - std::max(0ll, scratch_bytes));
}

} // namespace gten
