// fsm_build.h -- builders of token automata in the pool format of include/gten_hip_fsm.h: a dense u16 `next` table
// of [states][n_vocab] entries and a u8 `flags` row.  Host C++ with no device call, shared by the command line program and -- through
// the flat gten_host_fsm_* exports of host/capi_fsm.cpp -- by Python.  Every builder appends its automaton to the pool as a new range
// of states and returns its start state; a refusal (< 0) leaves the pool as it was.
#pragma once

#include <cstdint>
#include <cstring>
#include <map>
#include <vector>

#include "../../include/gten_hip_fsm.h"

namespace gten {

class FsmPool {
public:
    enum : int { kBadArgument = -1, kTooLarge = -2, kPrefix = -3 };

    explicit FsmPool(int n_vocab) : V_{n_vocab} {}
    int n_vocab() const { return V_; }
    int n_states() const { return (int)flags_.size(); }
    const uint16_t* next() const { return next_.data(); }
    const uint8_t* flags() const { return flags_.data(); }

    // Aho-Corasick over the n id sequences ids[offsets[k], offsets[k + 1]): nothing is banned, a state is final where any sequence
    // ends (so walking any id string from the start state is final exactly after the first position at which a sequence ends).
    int add_stop(const int32_t* ids, const int32_t* offsets, int n)
    {
        Trie t;
        if (const int rc = t.build(ids, offsets, n, V_, false)) return rc;
        const int S = (int)t.kids.size();
        if (!fits(S)) return kTooLarge;
        // failure links breadth first; a state's row is its failure state's row with its own edges on top
        std::vector<int> fail((size_t)S, 0), order;
        std::vector<uint16_t> rows((size_t)S * (size_t)V_, 0);
        std::vector<uint8_t> fin(t.ends.begin(), t.ends.end());
        order.reserve((size_t)S);
        for (const auto& e : t.kids[0]) { rows[(size_t)e.first] = (uint16_t)e.second; order.push_back(e.second); }
        for (size_t head = 0; head < order.size(); head++) {
            const int s = order[head], f = fail[(size_t)s];
            uint16_t* row = rows.data() + (size_t)s * (size_t)V_;
            std::memcpy(row, rows.data() + (size_t)f * (size_t)V_, (size_t)V_ * sizeof(uint16_t));
            if (fin[(size_t)f]) fin[(size_t)s] = 1;
            for (const auto& e : t.kids[(size_t)s]) {
                fail[(size_t)e.second] = (int)rows[(size_t)f * (size_t)V_ + (size_t)e.first];
                row[(size_t)e.first] = (uint16_t)e.second;
                order.push_back(e.second);
            }
        }
        return append(rows, fin, S);
    }

    // A trie over the n choices: in every state only the trie's edges are allowed, and the last id of a choice enters a final state.
    // A choice that is empty, or a prefix of another (or equal to one), is refused.
    int add_choices(const int32_t* ids, const int32_t* offsets, int n)
    {
        Trie t;
        if (const int rc = t.build(ids, offsets, n, V_, true)) return rc;
        const int S = (int)t.kids.size();
        if (!fits(S)) return kTooLarge;
        std::vector<uint16_t> rows((size_t)S * (size_t)V_, (uint16_t)GTEN_HIP_FSM_DEAD);
        for (int s = 0; s < S; s++)
            for (const auto& e : t.kids[(size_t)s]) rows[(size_t)s * (size_t)V_ + (size_t)e.first] = (uint16_t)e.second;
        return append(rows, std::vector<uint8_t>(t.ends.begin(), t.ends.end()), S);
    }

    // The caller's own automaton of S states (next [S][n_vocab] with entries below S or DEAD, flags [S]), relocated into the pool.
    int add_table(const uint16_t* next, const uint8_t* flags, int S)
    {
        if (!next || !flags || S < 1) return kBadArgument;
        if (!fits(S)) return kTooLarge;
        const std::vector<uint16_t> rows(next, next + (size_t)S * (size_t)V_);
        for (const uint16_t e : rows)
            if (e != GTEN_HIP_FSM_DEAD && e >= S) return kBadArgument;
        return append(rows, std::vector<uint8_t>(flags, flags + S), S);
    }

private:
    struct Trie {
        std::vector<std::map<int32_t, int>> kids{1};
        std::vector<char> ends{0};
        int build(const int32_t* ids, const int32_t* offsets, int n, int V, bool prefix_free)
        {
            if (!offsets || n < 1 || offsets[0] != 0) return kBadArgument;
            for (int k = 0; k < n; k++) {
                const int lo = offsets[k], hi = offsets[k + 1];
                if (hi <= lo || !ids) return kBadArgument;                       // (an empty sequence)
                int s = 0;
                for (int i = lo; i < hi; i++) {
                    if (ids[i] < 0 || ids[i] >= V) return kBadArgument;
                    if (prefix_free && ends[(size_t)s]) return kPrefix;          // (an earlier choice is a prefix of this one)
                    auto it = kids[(size_t)s].find(ids[i]);
                    if (it == kids[(size_t)s].end()) {
                        if (kids.size() >= (size_t)GTEN_HIP_FSM_MAX_STATES) return kTooLarge;
                        kids[(size_t)s][ids[i]] = (int)kids.size();
                        s = (int)kids.size();
                        kids.emplace_back();
                        ends.push_back(0);
                    } else {
                        s = it->second;
                    }
                }
                if (prefix_free && (ends[(size_t)s] || !kids[(size_t)s].empty())) return kPrefix;   // (equal to, or a prefix of, an earlier one)
                ends[(size_t)s] = 1;
            }
            return 0;
        }
    };

    bool fits(int S) const
    {
        const unsigned long long total = (unsigned long long)n_states() + (unsigned long long)S;
        return V_ >= 1 && total <= GTEN_HIP_FSM_MAX_STATES && total * (unsigned long long)V_ * 2ull <= GTEN_HIP_FSM_MAX_BYTES;
    }
    // `rows` (entries relative to the automaton's own state 0) become states [base, base + S) of the pool
    int append(const std::vector<uint16_t>& rows, const std::vector<uint8_t>& fin, int S)
    {
        const int base = n_states();
        next_.reserve(next_.size() + rows.size());
        for (const uint16_t e : rows) next_.push_back(e == GTEN_HIP_FSM_DEAD ? e : (uint16_t)(e + base));
        static_assert(GTEN_HIP_FSM_FINAL == 1, "the builders mark a final state with 1");
        flags_.insert(flags_.end(), fin.begin(), fin.begin() + S);
        return base;
    }

    int V_;
    std::vector<uint16_t> next_;
    std::vector<uint8_t> flags_;
};

} // namespace gten
