// fsm_build.h -- builders of token automata in the pool format of include/gten_hip_fsm.h: a dense u16 `next` table
// of [states][n_vocab] entries and a u8 `flags` row.  Host C++ with no device call, shared by the command line program and -- through
// the flat gten_host_fsm_* exports of host/capi_fsm.cpp -- by Python.  Every builder appends its automaton to the pool as a new range
// of states and returns its start state; a refusal (< 0) leaves the pool as it was.
//
// A regular expression (add_regex; host/regex_build.h) is kept as its byte automaton only -- a few KB instead of
// 2 * n_vocab bytes per state.  The pool is then a list of PARTS: ranges of host rows (packed in next_) and ranges that are byte
// automata.  next() materialises the latter with the host expansion (regex_expand: the definition the device's expansion is held to);
// a pool with no such range is one part, and next() is the table it always was.
//
// Stop strings given as text (add_stop_text; host/stop_text_build.h) are kept the same way, as a byte automaton in
// SEARCH mode: its token-level meaning is search_expand(), not regex_expand().
#pragma once

#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/gten_hip_fsm.h"
#include "regex_build.h"
#include "stop_text_build.h"

namespace gten {

class FsmPool {
public:
    enum : int { kBadArgument = -1, kTooLarge = -2, kPrefix = -3, kUnsupported = -4 };

    // states [first, first + count): host rows at next_[rows_at ...] (regex < 0), or byte automaton number `regex`
    struct Part { int first, count; size_t rows_at; int regex; };
    // a byte automaton and the rule that expands it: kMatch (regex_expand, with eos) or kSearch (search_expand, no eos)
    enum : int { kMatch = 0, kSearch = 1 };
    struct Regex { ByteDfa dfa; int eos; int mode = kMatch; };

    explicit FsmPool(int n_vocab) : V_{n_vocab} {}
    int n_vocab() const { return V_; }
    int n_states() const { return (int)flags_.size(); }
    // the whole pool as one table (valid until the next add): with regex ranges, the host expansion of each beside the host rows
    const uint16_t* next() const
    {
        if (regexes_.empty()) return next_.data();
        if (view_.empty()) {
            view_.resize((size_t)n_states() * (size_t)V_);
            for (const Part& p : parts_) {
                uint16_t* to = view_.data() + (size_t)p.first * (size_t)V_;
                if (p.regex < 0) std::memcpy(to, next_.data() + p.rows_at, (size_t)p.count * (size_t)V_ * sizeof(uint16_t));
                else if (regexes_[(size_t)p.regex].mode == kSearch) search_expand(regexes_[(size_t)p.regex].dfa, bytes_.data(), offsets_.data(), V_, p.first, to);
                else regex_expand(regexes_[(size_t)p.regex].dfa, bytes_.data(), offsets_.data(), V_, regexes_[(size_t)p.regex].eos, p.first, to);
            }
        }
        return view_.data();
    }
    const uint8_t* flags() const { return flags_.data(); }
    bool has_regex() const { return !regexes_.empty(); }
    const std::vector<Part>& parts() const { return parts_; }
    const Regex& regex(int i) const { return regexes_[(size_t)i]; }
    const uint16_t* host_rows(const Part& p) const { return next_.data() + p.rows_at; }
    bool has_vocab() const { return !offsets_.empty(); }
    const uint8_t* vocab_bytes() const { return bytes_.data(); }
    const int32_t* vocab_offsets() const { return offsets_.data(); }

    // The vocabulary as byte strings: id i spells bytes[offsets[i], offsets[i + 1]).  Refused once a regex or search range exists.
    int set_vocab(const uint8_t* bytes, const int32_t* offsets)
    {
        if (!offsets || offsets[0] != 0 || !regexes_.empty()) return kBadArgument;
        for (int i = 0; i < V_; i++)
            if (offsets[i + 1] < offsets[i]) return kBadArgument;
        if (offsets[V_] > 0 && !bytes) return kBadArgument;
        offsets_.assign(offsets, offsets + V_ + 1);
        bytes_.assign(bytes, bytes + offsets[V_]);
        bytes_.push_back(0);                 // (never empty: data() is a pointer)
        return 0;
    }

    // The pattern's byte automaton (regex_compile) as a range of Sb states, and the END state behind them when eos >= 0; the start
    // state.  An identical (pattern, eos) of this pool gives the range it already has.  *error_offset (may be NULL): where a refused
    // pattern offends, or -1.
    int add_regex(const char* pattern, size_t n, int eos, int* error_offset)
    {
        if (error_offset) *error_offset = -1;
        if (!pattern || !has_vocab() || eos < -1 || eos >= V_) return kBadArgument;
        const std::pair<std::string, int> key{std::string(pattern, n), eos};
        const auto it = regex_start_.find(key);
        if (it != regex_start_.end()) return it->second;
        Regex r{ByteDfa{}, eos};
        if (const int rc = regex_compile(pattern, n, r.dfa, error_offset)) return rc;
        const int count = regex_pool_states(r.dfa, eos), base = n_states();
        if (!fits(count)) return kTooLarge;
        flags_.resize((size_t)(base + count));
        regex_flags(r.dfa, eos, flags_.data() + base);
        parts_.push_back(Part{base, count, 0, (int)regexes_.size()});
        regexes_.push_back(std::move(r));
        regex_start_.emplace(key, base);
        view_.clear();
        return base;
    }

    // Stop strings as TEXT: the Aho-Corasick automaton of the n byte strings (stop_text_build) as a SEARCH range of Sb + 1 states, the
    // last one the HIT state; the start state.  Nothing is banned: up to the hit the ids are the unbound generation's, and the id
    // whose bytes complete a string -- wherever in its piece -- enters the HIT state, which is FINAL.
    int add_stop_text(const StopText* strings, int n)
    {
        if (!has_vocab()) return kBadArgument;
        Regex r{ByteDfa{}, -1, kSearch};
        if (const int rc = stop_text_build(strings, n, r.dfa)) return rc;
        const int count = search_pool_states(r.dfa), base = n_states();
        if (!fits(count)) return kTooLarge;
        flags_.resize((size_t)(base + count));
        search_flags(r.dfa, flags_.data() + base);
        parts_.push_back(Part{base, count, 0, (int)regexes_.size()});
        regexes_.push_back(std::move(r));
        view_.clear();
        return base;
    }

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
        if (!parts_.empty() && parts_.back().regex < 0) parts_.back().count += S;        // (host rows behind host rows: one part)
        else parts_.push_back(Part{base, S, next_.size(), -1});
        view_.clear();
        next_.reserve(next_.size() + rows.size());
        for (const uint16_t e : rows) next_.push_back(e == GTEN_HIP_FSM_DEAD ? e : (uint16_t)(e + base));
        static_assert(GTEN_HIP_FSM_FINAL == 1, "the builders mark a final state with 1");
        flags_.insert(flags_.end(), fin.begin(), fin.begin() + S);
        return base;
    }

    int V_;
    std::vector<uint16_t> next_;            // the rows of the host parts, packed
    std::vector<uint8_t> flags_;            // of every state
    std::vector<Part> parts_;
    std::vector<Regex> regexes_;
    std::map<std::pair<std::string, int>, int> regex_start_;
    std::vector<uint8_t> bytes_;
    std::vector<int32_t> offsets_;
    mutable std::vector<uint16_t> view_;    // next()'s table while regex ranges exist
};

} // namespace gten
