// stop_text_build.h -- stop strings given as TEXT: the Aho-Corasick automaton of a set of byte strings, and the place of the first
// match in a text.  Host C++ with no device call, in the manner of host/regex_build.h, whose ByteDfa it fills.
//
// stop_text_build() gives the automaton over BYTES in the ByteDfa format: u16 next[Sb][256], u8 accept[Sb], state 0 the start.
//   States: the trie's nodes, numbered breadth first from the root with bytes ascending -- CANONICAL: equal sets of strings give
//     equal tables, whatever their order and however often a string is repeated.
//   Edges: next[s][b] is TOTAL -- the goto function completed through the failure links; no entry is kNoEdge.
//   Acceptance: accept[s] = 1 where some string is a suffix of the path to s (its own end, or one reached through failure links).
// Refused with kStopTextBad (-1): no strings, a null pointer, an empty string.  kStopTextTooLarge (-2): more than kStopTextMaxNodes
// trie nodes (the pool's 65535 states, less the HIT state search_expand() adds and DEAD's own number).
//
// The automaton SEARCHES: it never dies, and a state is accepting exactly when a stop string has just ended.  Its token-level
// meaning is search_expand() of host/regex_build.h -- not regex_expand(), whose rule ("the walk survives every byte, final only
// where nothing can follow") would either never end or ban every piece that runs past the string.
//
// stop_text_find() tells a caller where to cut: of all occurrences of any string in the text, the one that ENDS first; among those
// that end at the same byte the LONGEST; among equal ones (a repeated string) the lowest index.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <vector>

#include "regex_build.h"

namespace gten {

enum : int { kStopTextBad = -1, kStopTextTooLarge = -2 };
constexpr int kStopTextMaxNodes = 65533;

// one stop string: n bytes at p, any byte allowed
struct StopText { const uint8_t* p; size_t n; };

inline int stop_text_build(const StopText* strings, int n, ByteDfa& out)
{
    if (!strings || n < 1) return kStopTextBad;
    for (int k = 0; k < n; k++)
        if (!strings[k].p || strings[k].n == 0) return kStopTextBad;
    // the trie, in the order the strings come
    std::vector<std::map<int, int>> kids(1);
    std::vector<uint8_t> ends(1, 0);
    for (int k = 0; k < n; k++) {
        int s = 0;
        for (size_t i = 0; i < strings[k].n; i++) {
            const int b = strings[k].p[i];
            const auto it = kids[(size_t)s].find(b);
            if (it != kids[(size_t)s].end()) { s = it->second; continue; }
            if ((int)kids.size() >= kStopTextMaxNodes) return kStopTextTooLarge;
            kids[(size_t)s][b] = (int)kids.size();
            s = (int)kids.size();
            kids.emplace_back();
            ends.push_back(0);
        }
        ends[(size_t)s] = 1;
    }
    // canonical numbers: breadth first, bytes ascending (std::map iterates so); order[new] = old
    const int S = (int)kids.size();
    std::vector<int> order, number((size_t)S, 0);
    order.reserve((size_t)S);
    order.push_back(0);
    for (size_t head = 0; head < order.size(); head++)
        for (const auto& e : kids[(size_t)order[head]]) {
            number[(size_t)e.second] = (int)order.size();
            order.push_back(e.second);
        }
    // failure links in the same order: a node's row is its failure node's row with its own edges on top
    out.next.assign((size_t)S * 256, 0);
    out.accept.assign((size_t)S, 0);
    std::vector<int> fail((size_t)S, 0);
    for (int s = 0; s < S; s++) {
        const int old = order[(size_t)s], f = fail[(size_t)s];
        uint16_t* row = out.next.data() + (size_t)s * 256;
        if (s > 0) std::memcpy(row, out.next.data() + (size_t)f * 256, 256 * sizeof(uint16_t));       // (f < s: it is shallower)
        out.accept[(size_t)s] = (ends[(size_t)old] || (s > 0 && out.accept[(size_t)f])) ? 1 : 0;
        for (const auto& e : kids[(size_t)old]) {
            const int kid = number[(size_t)e.second];
            fail[(size_t)kid] = s > 0 ? (int)row[e.first] : 0;          // (row still holds the failure node's edge here)
            row[e.first] = (uint16_t)kid;
        }
    }
    return 0;
}

struct StopTextHit { int index; long long begin, end; };

// the first match of any of the n strings in text[0, len): see the top of this file; no match (or nothing to look for): (-1, len, len)
inline StopTextHit stop_text_find(const StopText* strings, int n, const uint8_t* text, long long len)
{
    if (!strings || n < 1 || !text) return StopTextHit{-1, len, len};
    for (long long end = 1; end <= len; end++) {
        int best = -1;
        for (int k = 0; k < n; k++) {
            const size_t m = strings[k].n;
            if (!strings[k].p || m == 0 || (long long)m > end) continue;
            if (std::memcmp(text + (end - (long long)m), strings[k].p, m) != 0) continue;
            if (best < 0 || m > strings[best].n) best = k;
        }
        if (best >= 0) return StopTextHit{best, end - (long long)strings[best].n, end};
    }
    return StopTextHit{-1, len, len};
}

} // namespace gten
