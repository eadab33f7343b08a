// host_sanitize_regex.cpp -- the regular-expression compiler and the host expansion (host/regex_build.h, host/fsm_build.h) as a
// stand-alone program for -fsanitize=address,undefined (tests/test_regex_cpu.py builds and runs it; no device, nothing from Python).
// It compiles good and refused patterns, expands the good ones over a small vocabulary with pieces of every length from 0 to 40
// bytes, and checks what it can check alone: the refusal codes, the pool's size after a refusal, a few acceptances, and that every
// entry of the expanded pool is a state of the pool or DEAD.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "host/fsm_build.h"

using namespace gten;

static int failures = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

static bool accepts(const ByteDfa& d, const char* s) { return regex_accepts(d, (const uint8_t*)s, std::strlen(s)); }

int main()
{
    const char* good[] = {"a", "a|b", "(ab)?", "a{3,}", "a{0}", "[a\\-\\]]+", ".", ".*", "\\d+\\.\\d*", "\\W\\w", "(a|ab)(c|bcd)", "[^a]b",
                          "\\{\"k\": [0-9]{1,3}\\}", "(a(b(c)?)*)+", "\xc3\xa9+", ".\xf0\x9f\x98\x80", "(a|b)*a(a|b){7}", "([a-z]{1,40} ){4}", "x{255}", "(|a)(|b)"};
    struct { const char* p; int code; int at; } bad[] = {
        {"", -1, 0}, {"()", -1, 0}, {"(a", -1, 0}, {"a)", -1, 1}, {"[]", -1, 1}, {"[a", -1, 0}, {"a**", -1, 2}, {"a{2,1}", -1, 1}, {"a\\", -1, 1}, {"\\xg", -1, 0},
        {"^a", -4, 0}, {"a$", -4, 1}, {"\\b", -4, 0}, {"(a)\\1", -4, 3}, {"(?=a)", -4, 0}, {"a*?", -4, 2}, {"a{256}", -4, 1}, {"[\xc3\xa9]", -4, 1},
        {"\\xff", -4, 0}, {"(a|b)*a(a|b){16}", -2, -1}, {"\xc3", -1, 0}, {"a\xc3(", -1, 1}};
    // a vocabulary of 97 ids: empty pieces, single bytes, pieces of 2 .. 40 bytes, a NUL byte, broken UTF-8
    std::vector<std::string> pieces = {"", "a", "b", "c", "ab", "abb", " ", "0", "12", "3.5", ".", "\n", std::string(1, '\0'), "\xc3", "\xa9", "\xc3\xa9",
                                       "\xf0\x9f", "\x98\x80", "{\"k\": ", "}", "xx", "aaaa"};
    for (int n = 2; n <= 40 && pieces.size() < 96; n++) pieces.push_back(std::string((size_t)n, n % 2 ? 'a' : 'x'));
    while (pieces.size() < 97) pieces.push_back("");
    std::vector<uint8_t> bytes;
    std::vector<int32_t> offsets{0};
    for (const std::string& p : pieces) {
        bytes.insert(bytes.end(), p.begin(), p.end());
        offsets.push_back((int32_t)bytes.size());
    }
    const int V = (int)pieces.size();

    FsmPool pool(V);
    int at = 0;
    EXPECT(pool.add_regex("a", 1, -1, &at) == FsmPool::kBadArgument);          // no vocabulary yet
    EXPECT(pool.set_vocab(bytes.data(), offsets.data()) == 0);
    const int32_t stop_ids[] = {1, 2}, stop_off[] = {0, 2};
    EXPECT(pool.add_stop(stop_ids, stop_off, 1) == 0);
    int ranges = 0;
    for (const char* p : good) {
        ByteDfa d;
        EXPECT(regex_compile(p, std::strlen(p), d, &at) == 0 && at == -1);
        EXPECT(d.n_states() >= 1 && d.next.size() == (size_t)d.n_states() * 256);
        for (const int eos : {-1, 0, V - 1}) {
            const int before = pool.n_states();
            const int start = pool.add_regex(p, std::strlen(p), eos, &at);
            EXPECT(start == before && pool.n_states() == before + regex_pool_states(d, eos));
            EXPECT(pool.add_regex(p, std::strlen(p), eos, &at) == start && pool.n_states() == before + regex_pool_states(d, eos));
            ranges++;
        }
    }
    const int32_t choice_ids[] = {4, 5}, choice_off[] = {0, 1, 2};
    EXPECT(pool.add_choices(choice_ids, choice_off, 2) >= 0);                  // host rows behind the regex ranges
    const int S = pool.n_states();
    for (const auto& b : bad) {
        ByteDfa d;
        at = 12345;
        EXPECT(regex_compile(b.p, std::strlen(b.p), d, &at) == b.code && at == b.at);
        EXPECT(pool.add_regex(b.p, std::strlen(b.p), -1, &at) == b.code && pool.n_states() == S);
    }
    EXPECT(pool.add_regex("a", 1, V, &at) == FsmPool::kBadArgument && pool.add_regex("a", 1, -2, &at) == FsmPool::kBadArgument);
    EXPECT(pool.set_vocab(bytes.data(), offsets.data()) == FsmPool::kBadArgument && pool.n_states() == S);
    // the materialised pool: every entry a state or DEAD, every flag 0 or 1
    const uint16_t* next = pool.next();
    size_t live = 0;
    for (size_t i = 0; i < (size_t)S * (size_t)V; i++) {
        EXPECT(next[i] == GTEN_HIP_FSM_DEAD || next[i] < S);
        live += next[i] != GTEN_HIP_FSM_DEAD;
    }
    EXPECT(live > 100 && (int)pool.parts().size() == ranges + 2);
    for (int s = 0; s < S; s++) EXPECT(pool.flags()[s] <= 1);
    // a few acceptances, broken UTF-8 among them
    ByteDfa d;
    EXPECT(regex_compile(".", 1, d, &at) == 0);
    EXPECT(accepts(d, "a") && accepts(d, "\xc3\xa9") && accepts(d, "\xf0\x9f\x98\x80") && !accepts(d, "\n") && !accepts(d, "") && !accepts(d, "\xc3"));
    EXPECT(!accepts(d, "\xc0\x80") && !accepts(d, "\xed\xa0\x80") && !accepts(d, "\xf4\x90\x80\x80") && !accepts(d, "\xff"));
    EXPECT(regex_compile("x{255}", 6, d, &at) == 0 && d.n_states() == 256 && accepts(d, std::string(255, 'x').c_str()) && !accepts(d, std::string(254, 'x').c_str()));
    // an automaton larger than one pass and one workgroup's share of states, over a piece longer than any of them
    EXPECT(regex_compile("([a-z]{1,40} ){4}", 17, d, &at) == 0 && d.n_states() > 64);
    std::vector<uint16_t> rows((size_t)regex_pool_states(d, 0) * (size_t)V);
    regex_expand(d, bytes.data(), offsets.data(), V, 0, 7, rows.data());
    EXPECT(rows[1] == 7 + d.next[(size_t)'a'] && rows[0] == GTEN_HIP_FSM_DEAD);
    if (failures) return 1;
    std::printf("host_sanitize_regex ok (%d ranges, %d states)\n", ranges, S);
    return 0;
}
