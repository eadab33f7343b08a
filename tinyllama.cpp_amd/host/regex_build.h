// regex_build.h -- regular expressions as byte automata, and their expansion over a vocabulary into the pool format of
// include/gten_hip_fsm.h.  Host C++ with no device call.
//
// regex_compile() turns a UTF-8 pattern into a deterministic BYTE automaton: u16 next[Sb][256] (0xFFFF: no edge), u8 accept[Sb],
// state 0 the start, a match always of the whole text.  The contract is Python's: a byte string b is accepted iff it is valid
// UTF-8 and re.fullmatch(pattern, b.decode(), re.ASCII) matches.
//
// The dialect.  Literals (non-ASCII ones as their UTF-8 bytes); a backslash in front of any ASCII punctuation; \n \t \r \f \v; \xHH
// below 0x80; \d \D \w \W \s \S (ASCII: [0-9], [A-Za-z0-9_], [ \t\n\r\f\v]); `.` (any code point but \n); bracket classes and ranges
// over ASCII with ^ (the escapes above are allowed inside, \d \w \s and their negations too; `-` first or last is itself); ( ),
// (?: ), | (an alternative may be empty); ? * + {m} {m,} {m,n} with every bound <= 255.  `.`, \D \W \S and negated classes consume one
// whole well-formed code point (no overlong form, no surrogate, nothing above U+10FFFF), so every accepted string is valid UTF-8.
// Refused with kRegexSyntax (-1) and the byte offset of the offence: an empty pattern, ( ) and [ ] left open or empty, a `]` first in a
// class, a range that runs backwards or ends in a class escape, a quantifier with nothing in front of it or behind another
// quantifier, a `{` that opens no {m} {m,} {m,n}, m > n, a dangling backslash, an unknown letter escape, a pattern whose language
// is empty.  Refused with kRegexUnsupported (-4): ^ $ \b \B \A \Z, back-references and other digit escapes, \a \u \U \N, (?= (?! (?<
// (?P (?# and inline flags, lazy and possessive quantifiers, a bound above 255, a non-ASCII character inside brackets, \xHH >= 0x80.
// kRegexTooLarge (-2): more than 65535 subset states.
//
// The construction: Thompson NFA over byte sets; subset construction over the pattern's byte classes; removal of the states that
// cannot reach acceptance; Hopcroft's minimisation; CANONICAL numbering, breadth first from the start with bytes ascending -- equal
// languages give equal tables.
//
// regex_expand() is the token-level meaning, the one definition the device kernel (csrc/gten_fsm_expand.h) is held to:
// a vocabulary is bytes[] plus offsets[n_vocab + 1], id i spells bytes[offsets[i], offsets[i + 1]).  A byte automaton of Sb states
// becomes token states [base, base + Sb) (and base + Sb, the END state, when eos >= 0) of a pool:
//   next[base + s][i] = base + delta*(s, bytes of i) when the walk survives every byte and the piece is not empty, else DEAD;
//   an accepting state with no outgoing byte edge is FINAL;
//   an accepting state with outgoing edges is not: its next[..][eos] = base + Sb, the END state, FINAL, whose row is all DEAD;
//   eos is DEAD in every other state, whatever its bytes; with eos = -1 there is no END state.
#pragma once

#include <algorithm>
#include <array>
#include <bitset>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

namespace gten {

enum : int { kRegexSyntax = -1, kRegexTooLarge = -2, kRegexUnsupported = -4 };
constexpr uint16_t kNoEdge = 0xFFFF;
constexpr int kRegexMaxStates = 65535;
constexpr int kRegexMaxRepeat = 255;

struct ByteDfa {
    std::vector<uint16_t> next;         // [n][256]
    std::vector<uint8_t> accept;        // [n]
    int n_states() const { return (int)accept.size(); }
    bool has_edge(int s) const
    {
        for (int b = 0; b < 256; b++)
            if (next[(size_t)s * 256 + (size_t)b] != kNoEdge) return true;
        return false;
    }
};

namespace regex_detail {

using ByteSet = std::bitset<256>;

struct Ast {
    enum Kind { Empty, Set, Cat, Alt, Repeat } kind = Empty;
    ByteSet set;                                    // Set: one byte out of these
    std::vector<std::unique_ptr<Ast>> kids;         // Cat, Alt: any number; Repeat: one
    int lo = 0, hi = 0;                             // Repeat: hi -1 is "no upper bound"
};
using AstP = std::unique_ptr<Ast>;

inline AstP mk(Ast::Kind k) { AstP a(new Ast); a->kind = k; return a; }
inline AstP mk_set(const ByteSet& s) { AstP a = mk(Ast::Set); a->set = s; return a; }
inline AstP mk_range(int lo, int hi)
{
    ByteSet s;
    for (int b = lo; b <= hi; b++) s.set((size_t)b);
    return mk_set(s);
}
inline AstP mk_cat(std::vector<AstP> v)
{
    AstP a = mk(Ast::Cat);
    a->kids = std::move(v);
    return a;
}

// one code point out of (the ASCII bytes in `ascii`) or, with `beyond`, any well-formed code point above U+007F
inline AstP code_point(const ByteSet& ascii, bool beyond)
{
    if (!beyond) return mk_set(ascii);
    AstP alt = mk(Ast::Alt);
    if (ascii.any()) alt->kids.push_back(mk_set(ascii));
    auto seq = [&](std::initializer_list<std::pair<int, int>> ranges) {
        std::vector<AstP> v;
        for (const auto& r : ranges) v.push_back(mk_range(r.first, r.second));
        alt->kids.push_back(mk_cat(std::move(v)));
    };
    seq({{0xC2, 0xDF}, {0x80, 0xBF}});
    seq({{0xE0, 0xE0}, {0xA0, 0xBF}, {0x80, 0xBF}});
    seq({{0xE1, 0xEC}, {0x80, 0xBF}, {0x80, 0xBF}});
    seq({{0xED, 0xED}, {0x80, 0x9F}, {0x80, 0xBF}});
    seq({{0xEE, 0xEF}, {0x80, 0xBF}, {0x80, 0xBF}});
    seq({{0xF0, 0xF0}, {0x90, 0xBF}, {0x80, 0xBF}, {0x80, 0xBF}});
    seq({{0xF1, 0xF3}, {0x80, 0xBF}, {0x80, 0xBF}, {0x80, 0xBF}});
    seq({{0xF4, 0xF4}, {0x80, 0x8F}, {0x80, 0xBF}, {0x80, 0xBF}});
    return alt;
}

inline ByteSet ascii_class(char c)       // d, w, s
{
    ByteSet s;
    if (c == 'd' || c == 'w') for (int b = '0'; b <= '9'; b++) s.set((size_t)b);
    if (c == 'w') {
        for (int b = 'a'; b <= 'z'; b++) s.set((size_t)b);
        for (int b = 'A'; b <= 'Z'; b++) s.set((size_t)b);
        s.set((size_t)'_');
    }
    if (c == 's') for (const char b : {' ', '\t', '\n', '\r', '\f', '\v'}) s.set((size_t)(unsigned char)b);
    return s;
}

inline ByteSet ascii_not(const ByteSet& s)
{
    ByteSet r;
    for (int b = 0; b < 128; b++) r.set((size_t)b, !s.test((size_t)b));
    return r;
}

struct Parser {
    const unsigned char* p;
    size_t n, at = 0;
    int err = 0;
    size_t err_at = 0;
    size_t nodes = 0;                   // Ast nodes made by repeats, bounded below

    bool fail(int code, size_t where)
    {
        if (!err) { err = code; err_at = where; }
        return false;
    }
    bool more() const { return at < n; }
    static bool punct(unsigned char c) { return c < 128 && c > 32 && !((c >= '0' && c <= '9') || (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z')); }
    static int hex(unsigned char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }

    // An escape at p[at] == '\\'.  *cls: 0 a single byte in *byte, else one of d D w W s S.
    bool escape(bool in_class, int* byte, char* cls)
    {
        const size_t start = at++;
        if (!more()) return fail(kRegexSyntax, start);
        const unsigned char c = p[at++];
        *cls = 0;
        switch (c) {
        case 'n': *byte = '\n'; return true;
        case 't': *byte = '\t'; return true;
        case 'r': *byte = '\r'; return true;
        case 'f': *byte = '\f'; return true;
        case 'v': *byte = '\v'; return true;
        case 'd': case 'D': case 'w': case 'W': case 's': case 'S': *cls = (char)c; return true;
        case 'x': {
            if (at + 2 > n || hex(p[at]) < 0 || hex(p[at + 1]) < 0) return fail(kRegexSyntax, start);
            *byte = hex(p[at]) * 16 + hex(p[at + 1]);
            at += 2;
            if (*byte >= 0x80) return fail(kRegexUnsupported, start);
            return true;
        }
        default: break;
        }
        if (punct(c) || c == ' ') { *byte = c; return true; }
        if (c >= 0x80) return fail(in_class ? kRegexUnsupported : kRegexSyntax, start);
        if ((c >= '0' && c <= '9') || c == 'b' || c == 'B' || c == 'A' || c == 'Z' || c == 'a' || c == 'u' || c == 'U' || c == 'N')
            return fail(kRegexUnsupported, start);
        return fail(kRegexSyntax, start);
    }

    AstP bracket()
    {
        const size_t open = at++;
        bool neg = false;
        if (more() && p[at] == '^') { neg = true; at++; }
        ByteSet set;
        bool beyond = false, any = false;
        if (more() && p[at] == ']') { fail(kRegexSyntax, at); return nullptr; }
        for (;;) {
            if (!more()) { fail(kRegexSyntax, open); return nullptr; }
            if (p[at] == ']') { at++; break; }
            const size_t item = at;
            int lo = 0;
            char cls = 0;
            if (p[at] == '\\') { if (!escape(true, &lo, &cls)) return nullptr; }
            else if (p[at] >= 0x80) { fail(kRegexUnsupported, at); return nullptr; }
            else lo = p[at++];
            any = true;
            if (cls) {
                const ByteSet c = ascii_class((char)(cls | 0x20));
                if (cls & 0x20) set |= c;
                else { set |= ascii_not(c); beyond = true; }
                if (at + 1 < n && p[at] == '-' && p[at + 1] != ']') { fail(kRegexSyntax, item); return nullptr; }
                continue;
            }
            if (at + 1 < n && p[at] == '-' && p[at + 1] != ']') {
                at++;
                int hi = 0;
                char hcls = 0;
                if (p[at] == '\\') { if (!escape(true, &hi, &hcls)) return nullptr; }
                else if (p[at] >= 0x80) { fail(kRegexUnsupported, at); return nullptr; }
                else hi = p[at++];
                if (hcls || hi < lo) { fail(kRegexSyntax, item); return nullptr; }
                for (int b = lo; b <= hi; b++) set.set((size_t)b);
            } else {
                set.set((size_t)lo);
            }
        }
        if (!any) { fail(kRegexSyntax, open); return nullptr; }
        if (neg) return code_point(ascii_not(set), !beyond);
        return code_point(set, beyond);
    }

    AstP atom()
    {
        const unsigned char c = p[at];
        if (c == '(') {
            const size_t open = at++;
            if (more() && p[at] == '?') {
                if (at + 1 < n && p[at + 1] == ':') at += 2;
                else { fail(kRegexUnsupported, open); return nullptr; }
            }
            if (more() && p[at] == ')') { fail(kRegexSyntax, open); return nullptr; }
            AstP inner = alternation(open + 1);
            if (!inner) return nullptr;
            if (!more() || p[at] != ')') { fail(kRegexSyntax, open); return nullptr; }
            at++;
            return inner;
        }
        if (c == '[') return bracket();
        if (c == '.') {
            at++;
            ByteSet nl;
            nl.set((size_t)'\n');
            return code_point(ascii_not(nl), true);
        }
        if (c == '\\') {
            int b = 0;
            char cls = 0;
            if (!escape(false, &b, &cls)) return nullptr;
            if (!cls) return mk_range(b, b);
            const ByteSet s = ascii_class((char)(cls | 0x20));
            return (cls & 0x20) ? mk_set(s) : code_point(ascii_not(s), true);
        }
        if (c == '^' || c == '$') { fail(kRegexUnsupported, at); return nullptr; }
        if (c == '*' || c == '+' || c == '?' || c == '{') { fail(kRegexSyntax, at); return nullptr; }
        at++;
        return mk_range(c, c);          // a literal byte: ASCII, or one byte of a non-ASCII character's UTF-8 (checked by the caller)
    }

    // {m} {m,} {m,n} at p[at] == '{'
    bool bounds(int* lo, int* hi)
    {
        const size_t open = at++;
        auto number = [&](int* v) {
            if (!more() || p[at] < '0' || p[at] > '9') return false;
            long long x = 0;
            while (more() && p[at] >= '0' && p[at] <= '9') { x = std::min<long long>(x * 10 + (p[at] - '0'), 1000000); at++; }
            *v = (int)x;
            return true;
        };
        if (!number(lo)) return fail(kRegexSyntax, open);
        *hi = *lo;
        if (more() && p[at] == ',') {
            at++;
            *hi = -1;
            if (more() && p[at] != '}' && !number(hi)) return fail(kRegexSyntax, open);
        }
        if (!more() || p[at] != '}') return fail(kRegexSyntax, open);
        at++;
        if (*hi >= 0 && *hi < *lo) return fail(kRegexSyntax, open);
        if (*lo > kRegexMaxRepeat || *hi > kRegexMaxRepeat) return fail(kRegexUnsupported, open);
        return true;
    }

    static size_t size_of(const Ast& a)
    {
        size_t s = 1;
        for (const AstP& k : a.kids) s += size_of(*k);
        return a.kind == Ast::Repeat ? s * (size_t)std::max(1, std::max(a.lo, a.hi)) : s;
    }

    AstP piece()
    {
        const size_t start = at;
        // a non-ASCII literal: all the bytes of one well-formed character, so that a quantifier behind it takes the whole of it
        AstP a;
        if (p[at] >= 0x80) {
            const unsigned char c = p[at];
            const size_t len = c >= 0xF0 ? 4 : c >= 0xE0 ? 3 : c >= 0xC0 ? 2 : 0;
            if (len == 0 || at + len > n) { fail(kRegexSyntax, at); return nullptr; }
            std::vector<AstP> v;
            for (size_t i = 0; i < len; i++) {
                if (i > 0 && (p[at + i] & 0xC0) != 0x80) { fail(kRegexSyntax, at); return nullptr; }
                v.push_back(mk_range(p[at + i], p[at + i]));
            }
            at += len;
            a = mk_cat(std::move(v));
        } else {
            a = atom();
        }
        if (!a) return nullptr;
        if (!more()) return a;
        int lo = 0, hi = 0;
        const unsigned char q = p[at];
        const size_t qat = at;
        if (q == '*') { lo = 0; hi = -1; at++; }
        else if (q == '+') { lo = 1; hi = -1; at++; }
        else if (q == '?') { lo = 0; hi = 1; at++; }
        else if (q == '{') { if (!bounds(&lo, &hi)) return nullptr; }
        else return a;
        if (more() && (p[at] == '?' || p[at] == '+')) { fail(kRegexUnsupported, at); return nullptr; }      // lazy, possessive
        if (more() && (p[at] == '*' || p[at] == '{')) { fail(kRegexSyntax, at); return nullptr; }           // a repeat of a repeat
        AstP r = mk(Ast::Repeat);
        r->lo = lo;
        r->hi = hi;
        r->kids.push_back(std::move(a));
        if (size_of(*r) > (1u << 20)) { fail(kRegexTooLarge, qat); return nullptr; }
        (void)start;
        return r;
    }

    AstP alternation(size_t)
    {
        AstP alt = mk(Ast::Alt);
        std::vector<AstP> cat;
        for (;;) {
            if (!more() || p[at] == ')' || p[at] == '|') {
                alt->kids.push_back(cat.empty() ? mk(Ast::Empty) : mk_cat(std::move(cat)));
                cat.clear();
                if (more() && p[at] == '|') { at++; continue; }
                break;
            }
            AstP x = piece();
            if (!x) return nullptr;
            cat.push_back(std::move(x));
        }
        if (alt->kids.size() == 1) return std::move(alt->kids[0]);
        return alt;
    }
};

// ---- Thompson NFA: a node has one byte-set edge (set >= 0) or up to two empty edges
struct Nfa {
    struct Node { int set = -1; int a = -1, b = -1; };
    std::vector<Node> nodes;
    std::vector<ByteSet> sets;
    bool too_large = false;

    int add()
    {
        if (nodes.size() >= (1u << 21)) { too_large = true; return 0; }
        nodes.emplace_back();
        return (int)nodes.size() - 1;
    }
    void eps(int from, int to)
    {
        Node& x = nodes[(size_t)from];
        if (x.a < 0) x.a = to;
        else x.b = to;
    }
    // the fragment of `t` between a fresh entry node and a fresh exit node (the exit has no edge yet)
    std::pair<int, int> build(const Ast& t)
    {
        if (too_large) return {0, 0};
        switch (t.kind) {
        case Ast::Empty: {
            const int s = add(), e = add();
            eps(s, e);
            return {s, e};
        }
        case Ast::Set: {
            const int s = add(), e = add();
            sets.push_back(t.set);
            nodes[(size_t)s].set = (int)sets.size() - 1;
            nodes[(size_t)s].a = e;
            return {s, e};
        }
        case Ast::Cat: {
            const int s = add();
            int cur = s;
            for (const AstP& k : t.kids) {
                const auto f = build(*k);
                eps(cur, f.first);
                cur = f.second;
            }
            const int e = add();
            eps(cur, e);
            return {s, e};
        }
        case Ast::Alt: {
            const int e = add();
            int s = add();
            const int first = s;
            for (size_t i = 0; i < t.kids.size(); i++) {
                const auto f = build(*t.kids[i]);
                eps(s, f.first);
                eps(f.second, e);
                if (i + 2 < t.kids.size()) {         // a chain of two-way forks
                    const int more = add();
                    eps(s, more);
                    s = more;
                }
            }
            return {first, e};
        }
        case Ast::Repeat: {
            const int s = add();
            int cur = s;
            for (int i = 0; i < t.lo; i++) {
                const auto f = build(*t.kids[0]);
                eps(cur, f.first);
                cur = f.second;
            }
            const int e = add();
            if (t.hi < 0) {                          // x*: a loop node
                const int loop = add();
                eps(cur, loop);
                const auto f = build(*t.kids[0]);
                eps(loop, f.first);
                eps(loop, e);
                const int back = f.second;
                eps(back, loop);
            } else {
                for (int i = t.lo; i < t.hi; i++) {  // (x(x(x)?)?)?
                    const int fork = add();
                    eps(cur, fork);
                    eps(fork, e);
                    const auto f = build(*t.kids[0]);
                    eps(fork, f.first);
                    cur = f.second;
                }
                eps(cur, e);
            }
            return {s, e};
        }
        }
        return {0, 0};
    }
};

// the partition of Hopcroft's algorithm
struct Partition {
    std::vector<int> elems, loc, block, begin, end;
    explicit Partition(int n) : elems((size_t)n), loc((size_t)n), block((size_t)n, 0)
    {
        for (int i = 0; i < n; i++) elems[(size_t)i] = loc[(size_t)i] = i;
        begin.push_back(0);
        end.push_back(n);
    }
    int n_blocks() const { return (int)begin.size(); }
    int size(int b) const { return end[(size_t)b] - begin[(size_t)b]; }
};

} // namespace regex_detail

// The pattern (n bytes of UTF-8) as a minimal byte automaton in canonical numbering: 0, or a refusal with *error_offset (may be NULL)
// the byte offset of the offence (-1 where it has none: too many states).
inline int regex_compile(const char* pattern, size_t n, ByteDfa& out, int* error_offset)
{
    using namespace regex_detail;
    if (error_offset) *error_offset = -1;
    auto refuse = [&](int code, long long where) {
        if (error_offset) *error_offset = (int)where;
        return code;
    };
    if (!pattern || n == 0) return refuse(kRegexSyntax, 0);
    Parser ps{(const unsigned char*)pattern, n};
    AstP ast = ps.alternation(0);
    if (!ast) return refuse(ps.err, (long long)ps.err_at);
    if (ps.more()) return refuse(kRegexSyntax, (long long)ps.at);       // an unbalanced `)`

    Nfa nfa;
    const auto whole = nfa.build(*ast);
    if (nfa.too_large) return refuse(kRegexTooLarge, -1);
    const int n_nfa = (int)nfa.nodes.size(), nfa_accept = whole.second;

    // byte classes: bytes that sit in exactly the same sets of the pattern move every state alike
    std::vector<int> cls_of(256, 0);
    std::vector<int> cls_rep;
    {
        std::map<std::vector<bool>, int> seen;
        for (int b = 0; b < 256; b++) {
            std::vector<bool> sig(nfa.sets.size());
            for (size_t i = 0; i < nfa.sets.size(); i++) sig[i] = nfa.sets[i].test((size_t)b);
            auto it = seen.find(sig);
            if (it == seen.end()) {
                it = seen.emplace(std::move(sig), (int)cls_rep.size()).first;
                cls_rep.push_back(b);
            }
            cls_of[(size_t)b] = it->second;
        }
    }
    const int C = (int)cls_rep.size();

    // subset construction
    std::vector<int> mark((size_t)n_nfa, -1), stack;
    int stamp = 0;
    auto closure = [&](std::vector<int>& set) {          // the nodes with a byte edge, and the accepting node, reachable by empty edges
        stamp++;
        stack.clear();
        for (const int x : set)
            if (mark[(size_t)x] != stamp) { mark[(size_t)x] = stamp; stack.push_back(x); }
        set.clear();
        while (!stack.empty()) {
            const int x = stack.back();
            stack.pop_back();
            const Nfa::Node& nd = nfa.nodes[(size_t)x];
            if (nd.set >= 0 || x == nfa_accept) { set.push_back(x); continue; }
            for (const int y : {nd.a, nd.b})
                if (y >= 0 && mark[(size_t)y] != stamp) { mark[(size_t)y] = stamp; stack.push_back(y); }
        }
        std::sort(set.begin(), set.end());
    };
    std::map<std::vector<int>, int> ids;
    std::vector<std::vector<int>> subsets;
    std::vector<int> trans;                               // [state][C], -1: none
    std::vector<uint8_t> acc;
    {
        std::vector<int> start{whole.first};
        closure(start);
        ids.emplace(start, 0);
        subsets.push_back(std::move(start));
    }
    std::vector<int> target;
    for (size_t s = 0; s < subsets.size(); s++) {
        trans.resize((s + 1) * (size_t)C, -1);
        acc.push_back(std::binary_search(subsets[s].begin(), subsets[s].end(), nfa_accept) ? 1 : 0);
        for (int c = 0; c < C; c++) {
            target.clear();
            const size_t b = (size_t)cls_rep[(size_t)c];
            for (const int x : subsets[s]) {
                const Nfa::Node& nd = nfa.nodes[(size_t)x];
                if (nd.set >= 0 && nfa.sets[(size_t)nd.set].test(b)) target.push_back(nd.a);
            }
            if (target.empty()) continue;
            closure(target);
            auto it = ids.find(target);
            if (it == ids.end()) {
                if (subsets.size() >= (size_t)kRegexMaxStates) return refuse(kRegexTooLarge, -1);
                it = ids.emplace(target, (int)subsets.size()).first;
                subsets.push_back(target);
            }
            trans[s * (size_t)C + (size_t)c] = it->second;
        }
    }
    const int D = (int)subsets.size();

    // states that reach acceptance (backwards from the accepting ones); the rest become the sink
    std::vector<std::vector<int>> back((size_t)D);
    for (int s = 0; s < D; s++)
        for (int c = 0; c < C; c++)
            if (trans[(size_t)s * (size_t)C + (size_t)c] >= 0) back[(size_t)trans[(size_t)s * (size_t)C + (size_t)c]].push_back(s);
    std::vector<char> live((size_t)D, 0);
    {
        std::vector<int> todo;
        for (int s = 0; s < D; s++)
            if (acc[(size_t)s]) { live[(size_t)s] = 1; todo.push_back(s); }
        while (!todo.empty()) {
            const int s = todo.back();
            todo.pop_back();
            for (const int q : back[(size_t)s])
                if (!live[(size_t)q]) { live[(size_t)q] = 1; todo.push_back(q); }
        }
    }
    if (!live[0]) return refuse(kRegexSyntax, 0);        // the language is empty

    // a total automaton over the live states plus one sink, numbered 0 .. L (the sink is L)
    std::vector<int> idx((size_t)D, -1);
    int L = 0;
    for (int s = 0; s < D; s++)
        if (live[(size_t)s]) idx[(size_t)s] = L++;
    const int T = L + 1;
    std::vector<int> step((size_t)T * (size_t)C, L);
    std::vector<uint8_t> tacc((size_t)T, 0);
    for (int s = 0; s < D; s++) {
        if (!live[(size_t)s]) continue;
        tacc[(size_t)idx[(size_t)s]] = acc[(size_t)s];
        for (int c = 0; c < C; c++) {
            const int t = trans[(size_t)s * (size_t)C + (size_t)c];
            if (t >= 0 && live[(size_t)t]) step[(size_t)idx[(size_t)s] * (size_t)C + (size_t)c] = idx[(size_t)t];
        }
    }

    // Hopcroft: inverse edges per class as one offset table
    std::vector<int> inv_off((size_t)T * (size_t)C + 1, 0), inv((size_t)T * (size_t)C);
    for (int s = 0; s < T; s++)
        for (int c = 0; c < C; c++) inv_off[(size_t)step[(size_t)s * (size_t)C + (size_t)c] * (size_t)C + (size_t)c + 1]++;
    for (size_t i = 1; i < inv_off.size(); i++) inv_off[i] += inv_off[i - 1];
    {
        std::vector<int> fill(inv_off.begin(), inv_off.end() - 1);
        for (int s = 0; s < T; s++)
            for (int c = 0; c < C; c++) inv[(size_t)fill[(size_t)step[(size_t)s * (size_t)C + (size_t)c] * (size_t)C + (size_t)c]++] = s;
    }
    Partition P(T);
    std::vector<int> work;
    std::vector<char> in_work;
    {
        // the first split: accepting | not
        int lo = 0;
        for (int i = 0; i < T; i++)
            if (tacc[(size_t)P.elems[(size_t)i]]) {
                const int x = P.elems[(size_t)i], y = P.elems[(size_t)lo];
                P.elems[(size_t)lo] = x; P.elems[(size_t)i] = y;
                P.loc[(size_t)x] = lo; P.loc[(size_t)y] = i;
                lo++;
            }
        if (lo > 0 && lo < T) {
            P.end[0] = lo;
            P.begin.push_back(lo);
            P.end.push_back(T);
            for (int i = lo; i < T; i++) P.block[(size_t)P.elems[(size_t)i]] = 1;
        }
        in_work.assign((size_t)P.n_blocks(), 1);
        for (int b = 0; b < P.n_blocks(); b++) work.push_back(b);
    }
    std::vector<int> members, touched, hit_count((size_t)T + 2, 0);
    while (!work.empty()) {
        const int A = work.back();
        work.pop_back();
        in_work[(size_t)A] = 0;
        members.assign(P.elems.begin() + P.begin[(size_t)A], P.elems.begin() + P.end[(size_t)A]);
        for (int c = 0; c < C; c++) {
            touched.clear();
            // move every predecessor to the front of its block
            for (const int q : members) {
                const size_t k = (size_t)q * (size_t)C + (size_t)c;
                for (int e = inv_off[k]; e < inv_off[k + 1]; e++) {
                    const int x = inv[(size_t)e], b = P.block[(size_t)x];
                    if ((size_t)b >= hit_count.size()) hit_count.resize((size_t)b + 1, 0);
                    const int front = P.begin[(size_t)b] + hit_count[(size_t)b];
                    if (P.loc[(size_t)x] < front) continue;              // (already moved)
                    if (hit_count[(size_t)b]++ == 0) touched.push_back(b);
                    const int y = P.elems[(size_t)front], lx = P.loc[(size_t)x];
                    P.elems[(size_t)front] = x; P.elems[(size_t)lx] = y;
                    P.loc[(size_t)x] = front; P.loc[(size_t)y] = lx;
                }
            }
            for (const int b : touched) {
                const int hits = hit_count[(size_t)b];
                hit_count[(size_t)b] = 0;
                if (hits == P.size(b)) continue;
                // the hit part [begin, begin + hits) becomes a new block
                const int nb = P.n_blocks();
                P.begin.push_back(P.begin[(size_t)b]);
                P.end.push_back(P.begin[(size_t)b] + hits);
                P.begin[(size_t)b] += hits;
                for (int i = P.begin[(size_t)nb]; i < P.end[(size_t)nb]; i++) P.block[(size_t)P.elems[(size_t)i]] = nb;
                in_work.push_back(0);
                if (hit_count.size() <= (size_t)nb) hit_count.resize((size_t)nb + 1, 0);
                const int add = in_work[(size_t)b] ? nb : (P.size(nb) <= P.size(b) ? nb : b);
                in_work[(size_t)add] = 1;
                work.push_back(add);
            }
        }
    }

    // canonical numbering: breadth first from the start's block, bytes ascending; the sink's block is left out
    const int sink_block = P.block[(size_t)L];
    std::vector<int> number((size_t)P.n_blocks(), -1), order;
    number[(size_t)P.block[0]] = 0;
    order.push_back(P.block[0]);
    out.next.clear();
    out.accept.clear();
    for (size_t head = 0; head < order.size(); head++) {
        const int rep = P.elems[(size_t)P.begin[(size_t)order[head]]];
        out.accept.push_back(tacc[(size_t)rep]);
        out.next.resize((head + 1) * 256, kNoEdge);
        for (int b = 0; b < 256; b++) {
            const int t = P.block[(size_t)step[(size_t)rep * (size_t)C + (size_t)cls_of[(size_t)b]]];
            if (t == sink_block) continue;
            if (number[(size_t)t] < 0) {
                number[(size_t)t] = (int)order.size();
                order.push_back(t);
            }
            out.next[head * 256 + (size_t)b] = (uint16_t)number[(size_t)t];
        }
    }
    return 0;
}

// whether the automaton accepts the n bytes (the contract's left side; used by the tests and the stand-alone checks)
inline bool regex_accepts(const ByteDfa& d, const uint8_t* bytes, size_t n)
{
    int s = 0;
    for (size_t i = 0; i < n; i++) {
        const uint16_t t = d.next[(size_t)s * 256 + bytes[i]];
        if (t == kNoEdge) return false;
        s = t;
    }
    return d.accept[(size_t)s] != 0;
}

// how many pool states the automaton takes with this eos: its own, and the END state when eos >= 0
inline int regex_pool_states(const ByteDfa& d, int eos) { return d.n_states() + (eos >= 0 ? 1 : 0); }

// the flags of those states, to flags[0 .. regex_pool_states)
inline void regex_flags(const ByteDfa& d, int eos, uint8_t* flags)
{
    for (int s = 0; s < d.n_states(); s++) flags[s] = (d.accept[(size_t)s] && !d.has_edge(s)) ? 1 : 0;
    if (eos >= 0) flags[d.n_states()] = 1;
}

// The host expansion: rows [0, regex_pool_states) of `rows` (u16 [..][n_vocab]; entries are pool states, base + the automaton's own)
// by the definition at the top of this file.  The reference the device kernel is held to.
inline void regex_expand(const ByteDfa& d, const uint8_t* bytes, const int32_t* offsets, int n_vocab, int eos, int base, uint16_t* rows)
{
    const int Sb = d.n_states();
    for (int s = 0; s < Sb; s++) {
        uint16_t* row = rows + (size_t)s * (size_t)n_vocab;
        for (int i = 0; i < n_vocab; i++) {
            int cur = s;
            const int lo = offsets[i], hi = offsets[i + 1];
            if (hi <= lo) cur = -1;
            for (int j = lo; j < hi && cur >= 0; j++) {
                const uint16_t t = d.next[(size_t)cur * 256 + bytes[j]];
                cur = t == kNoEdge ? -1 : (int)t;
            }
            row[i] = cur < 0 ? (uint16_t)0xFFFF : (uint16_t)(base + cur);
        }
        if (eos >= 0 && eos < n_vocab) row[eos] = (d.accept[(size_t)s] && d.has_edge(s)) ? (uint16_t)(base + Sb) : (uint16_t)0xFFFF;
    }
    if (eos >= 0) std::fill(rows + (size_t)Sb * (size_t)n_vocab, rows + (size_t)(Sb + 1) * (size_t)n_vocab, (uint16_t)0xFFFF);
}

// The token-level meaning of a SEARCH automaton (host/stop_text_build.h): one that looks for something in the text
// and bans nothing on the way.  Sb byte states become pool states [base, base + Sb], always Sb + 1 of them: base + Sb is the HIT
// state, FINAL, whose row is all DEAD; the flags of the others are 0.  For s < Sb and id i:
//   an empty piece stays: next[base + s][i] = base + s (ids beyond the tokenizer, control ids, eos: nothing is banned);
//   a non-empty piece walks its bytes from s: base + Sb if the state after ANY byte is accepting, else base + the last state;
//   an entry >= Sb of the automaton reads as "no edge" and makes the entry DEAD (a built automaton has none).
// The rows of accepting byte states are written by the same rule and are unreachable.  rows: u16 [Sb + 1][n_vocab].  The reference the
// device kernel (csrc/gten_fsm_search.h) is held to, byte for byte.
inline int search_pool_states(const ByteDfa& d) { return d.n_states() + 1; }

inline void search_flags(const ByteDfa& d, uint8_t* flags)
{
    std::fill(flags, flags + d.n_states(), (uint8_t)0);
    flags[d.n_states()] = 1;
}

inline void search_expand(const ByteDfa& d, const uint8_t* bytes, const int32_t* offsets, int n_vocab, int base, uint16_t* rows)
{
    const int Sb = d.n_states();
    for (int s = 0; s < Sb; s++) {
        uint16_t* row = rows + (size_t)s * (size_t)n_vocab;
        for (int i = 0; i < n_vocab; i++) {
            int cur = s;
            bool hit = false;
            for (int j = offsets[i]; j < offsets[i + 1] && cur >= 0; j++) {
                const uint16_t t = d.next[(size_t)cur * 256 + bytes[j]];
                cur = (int)t < Sb ? (int)t : -1;
                if (cur >= 0 && d.accept[(size_t)cur]) hit = true;
            }
            row[i] = cur < 0 ? (uint16_t)0xFFFF : (uint16_t)(base + (hit ? Sb : cur));
        }
    }
    std::fill(rows + (size_t)Sb * (size_t)n_vocab, rows + (size_t)(Sb + 1) * (size_t)n_vocab, (uint16_t)0xFFFF);
}

} // namespace gten
