// prefix_match.h -- which registered prefix a prompt takes (include/gten_host_prefixes.h, DESIGN.md 3.9 "several prefixes").  No
// device, no gten type: plain ids in, an index out -- host/tinyllama_model.h asks it for every prompt, tests/test_prefixes_cpu.py
// checks it against a Python restatement.
#pragma once

#include <cstddef>
#include <cstdint>

namespace gten {

// a prompt must have at least this many ids of its own behind a prefix to take the short way (a segment of the row matrix has
// at least 16 rows)
constexpr int kPrefixOwnMin = 16;
// prefixes a batch and its shared decoder hold at the same time (GTEN_PREFIXES_MAX of include/gten_hip_prefixes.h)
constexpr int kPrefixesMax = 8;

// The index of the LONGEST prefix (ids[i], lens[i] > 0; lens[i] <= 0: index i is not registered) that prompt[0, n) begins with
// and has at least kPrefixOwnMin ids behind; -1: none.  Two matching prefixes of the same length hold the same ids: the lower
// index wins.
inline int prefixes_match_ptrs(const int32_t* const* ids, const int* lens, int n_prefixes, const int32_t* prompt, int n)
{
    int best = -1, best_len = 0;
    for (int i = 0; i < n_prefixes; i++) {
        const int len = lens[i];
        if (len <= best_len || !ids[i] || (long long)len + kPrefixOwnMin > (long long)n) continue;
        bool same = true;
        for (int j = 0; j < len && same; j++) same = ids[i][j] == prompt[j];
        if (same) { best = i; best_len = len; }
    }
    return best;
}

// the same over one array: prefix i's ids are prefix_ids[i * max_len .. i * max_len + lens[i]) (lens[i] <= max_len)
inline int prefixes_match(const int32_t* prefix_ids, const int* lens, int n_prefixes, int max_len, const int32_t* prompt, int n)
{
    if (n_prefixes <= 0 || n_prefixes > 64 || !prefix_ids || !lens || !prompt || max_len < 0 || n < 0) return -1;
    const int32_t* ids[64];
    for (int i = 0; i < n_prefixes; i++) ids[i] = lens[i] > 0 && lens[i] <= max_len ? prefix_ids + (size_t)i * (size_t)max_len : nullptr;
    return prefixes_match_ptrs(ids, lens, n_prefixes, prompt, n);
}

} // namespace gten
