// host_text_automata.cpp -- stop strings as text and JSON schemas as patterns (host/stop_text_build.h, host/json_schema.h,
// host/regex_build.h, host/fsm_build.h) as a stand-alone program for -fsanitize=address,undefined (tests/test_stoptext_cpu.py builds and
// runs it; no device, nothing from Python).  It builds the automata of the tests' string sets and refused ones, expands them over a
// small vocabulary, finds matches, compiles good, refused, malformed and truncated schemas -- every prefix of a good schema among them --
// and compiles the patterns of the good ones; it checks what it can check alone.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "host/fsm_build.h"
#include "host/json_schema.h"

using namespace gten;

static int failures = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

static std::vector<StopText> texts(const std::vector<std::string>& v)
{
    std::vector<StopText> out;
    for (const std::string& s : v) out.push_back(StopText{(const uint8_t*)s.data(), s.size()});
    return out;
}

int main()
{
    // ---- the automaton
    const std::vector<std::vector<std::string>> sets = {{"a"}, {"abcab", "ab"}, {"aba", "bab"}, {"\nUser:", "</answer>", "</a"},
                                                        {"\xff\x80", "\x80\xff\x80", std::string(1, '\0'), std::string("a\0b", 3)}, {"aaaa", "aa", "a"}};
    for (const auto& set : sets) {
        ByteDfa d, e;
        const std::vector<StopText> t = texts(set);
        EXPECT(stop_text_build(t.data(), (int)t.size(), d) == 0);
        EXPECT(d.n_states() >= 2 && d.next.size() == (size_t)d.n_states() * 256 && !d.accept[0]);
        for (const uint16_t x : d.next) EXPECT(x < d.n_states());                              // total
        std::vector<StopText> back(t.rbegin(), t.rend());
        back.push_back(t[0]);
        EXPECT(stop_text_build(back.data(), (int)back.size(), e) == 0 && e.next == d.next && e.accept == d.accept);      // canonical
        // acceptance is "a string has just ended", on a text made of the strings themselves
        std::string text;
        for (int r = 0; r < 3; r++)
            for (const std::string& s : set) text += s + s.substr(0, s.size() / 2);
        int s = 0;
        for (size_t k = 0; k < text.size(); k++) {
            s = d.next[(size_t)s * 256 + (uint8_t)text[k]];
            bool ends = false;
            for (const std::string& x : set) ends |= k + 1 >= x.size() && text.compare(k + 1 - x.size(), x.size(), x) == 0;
            EXPECT((d.accept[(size_t)s] != 0) == ends);
        }
        const StopTextHit h = stop_text_find(t.data(), (int)t.size(), (const uint8_t*)text.data(), (long long)text.size());
        EXPECT(h.index >= 0 && h.end - h.begin == (long long)set[(size_t)h.index].size() && h.end <= (long long)text.size());
    }
    {
        ByteDfa d;
        const StopText none{nullptr, 0}, empty{(const uint8_t*)"", 0};
        EXPECT(stop_text_build(nullptr, 0, d) == kStopTextBad && stop_text_build(&none, 1, d) == kStopTextBad && stop_text_build(&empty, 1, d) == kStopTextBad);
        const std::string a(32767, 'a'), b(32766, 'b'), c(32766, 'a');
        const std::vector<std::string> big_set = {a, b}, fits_set = {c, b}, tie_set = {"b", "ab", "aab"};
        const std::vector<StopText> big = texts(big_set), fits = texts(fits_set);
        EXPECT(stop_text_build(big.data(), 2, d) == kStopTextTooLarge);
        EXPECT(stop_text_build(fits.data(), 2, d) == 0 && d.n_states() == kStopTextMaxNodes);
        const std::vector<StopText> t = texts(tie_set);
        StopTextHit h = stop_text_find(t.data(), 3, (const uint8_t*)"xaab", 4);
        EXPECT(h.index == 2 && h.begin == 1 && h.end == 4);
        h = stop_text_find(t.data(), 3, (const uint8_t*)"xyz", 3);
        EXPECT(h.index == -1 && h.begin == 3 && h.end == 3);
        h = stop_text_find(t.data(), 3, (const uint8_t*)"", 0);
        EXPECT(h.index == -1 && h.begin == 0 && h.end == 0);
    }

    // ---- the expansion, in a pool beside the other kinds of range
    std::vector<std::string> pieces = {"", "a", "b", "c", "</", "", "answer>", "x", "<</answer>yy", "..</answer>", "abc</ans", "wer>abc", "\xc3\xa9", "",
                                       "{", "}", "\"", ":", ",", "t", "r", "u", "e", "f", "l", "s", "true", "\"}", "\":", "1", "0", "[", "]", "}]", "n"};
    for (int n = 2; n <= 40; n++) pieces.push_back(std::string((size_t)n, n % 2 ? 'a' : 'b') + "ab");
    std::vector<uint8_t> bytes;
    std::vector<int32_t> offsets{0};
    for (const std::string& p : pieces) {
        bytes.insert(bytes.end(), p.begin(), p.end());
        offsets.push_back((int32_t)bytes.size());
    }
    const int V = (int)pieces.size();
    FsmPool pool(V);
    const std::vector<std::string> stop_set = {"</answer>", "abcab", "ab"};
    const std::vector<StopText> stops = texts(stop_set);
    EXPECT(pool.add_stop_text(stops.data(), 3) == FsmPool::kBadArgument);                      // no vocabulary yet
    EXPECT(pool.set_vocab(bytes.data(), offsets.data()) == 0);
    const int32_t stop_ids[] = {1, 2}, stop_off[] = {0, 2};
    EXPECT(pool.add_stop(stop_ids, stop_off, 1) == 0);
    const int base = pool.add_stop_text(stops.data(), 3);
    ByteDfa d;
    EXPECT(stop_text_build(stops.data(), 3, d) == 0);
    const int Sb = d.n_states();
    EXPECT(base == 3 && pool.n_states() == base + Sb + 1);
    EXPECT(pool.add_stop_text(stops.data(), 0) == kStopTextBad && pool.n_states() == base + Sb + 1);
    EXPECT(pool.set_vocab(bytes.data(), offsets.data()) == FsmPool::kBadArgument);
    int at = 0;
    const int re = pool.add_regex("[ab]+c", 6, 0, &at);
    EXPECT(re == base + Sb + 1);
    {
        const uint16_t* next = pool.next();
        const int S = pool.n_states();
        for (size_t i = 0; i < (size_t)S * (size_t)V; i++) EXPECT(next[i] == GTEN_HIP_FSM_DEAD || next[i] < S);
        for (int s = 0; s < Sb; s++) {
            EXPECT(pool.flags()[base + s] == 0);
            for (int i = 0; i < V; i++) EXPECT(next[(size_t)(base + s) * (size_t)V + (size_t)i] >= base && next[(size_t)(base + s) * (size_t)V + (size_t)i] <= base + Sb);
            EXPECT(next[(size_t)(base + s) * (size_t)V] == base + s);                          // an empty piece stays
        }
        EXPECT(pool.flags()[base + Sb] == 1);
        for (int i = 0; i < V; i++) EXPECT(next[(size_t)(base + Sb) * (size_t)V + (size_t)i] == GTEN_HIP_FSM_DEAD);
        EXPECT(next[(size_t)base * (size_t)V + 8] == base + Sb && next[(size_t)base * (size_t)V + 9] == base + Sb);
        const int mid = next[(size_t)base * (size_t)V + 4];                                    // "</" then "answer>": the string straddles the pair
        EXPECT(mid != base + Sb && mid != base && next[(size_t)mid * (size_t)V + 6] == base + Sb && next[(size_t)base * (size_t)V + 6] != base + Sb);
    }
    // an automaton with entries outside itself: read as "no edge", DEAD, nothing out of bounds
    {
        ByteDfa odd = d;
        odd.next[(size_t)'a'] = (uint16_t)Sb;
        odd.next[(size_t)'b'] = 0xFFFF;
        std::vector<uint16_t> rows((size_t)(Sb + 1) * (size_t)V);
        search_expand(odd, bytes.data(), offsets.data(), V, 5, rows.data());
        EXPECT(rows[1] == GTEN_HIP_FSM_DEAD && rows[2] == GTEN_HIP_FSM_DEAD && rows[0] == 5 && rows[3] == 5);
    }

    // ---- schemas
    const char* good[] = {
        "{}", "{\"type\": \"string\"}", "{\"type\": \"string\", \"minLength\": 2, \"maxLength\": 5}", "{\"type\": [\"integer\", \"null\"]}",
        "{\"type\": \"number\"}", "{\"enum\": [\"a.b\", 3, -7, true, null, \"q\\\"\\\\\\n\\u00e9\\ud83d\\ude00\"]}", "{\"const\": \"x|y\"}",
        "{\"type\": \"array\", \"items\": {\"type\": \"integer\"}, \"minItems\": 1, \"maxItems\": 3}", "{\"type\": \"array\", \"maxItems\": 0}",
        "{\"type\": \"array\"}", "{\"type\": \"array\", \"items\": {\"type\": \"boolean\"}, \"minItems\": 2}",
        "{\"type\": \"object\", \"properties\": {\"a\": {\"type\": \"integer\"}, \"b\": {\"type\": \"string\"}, \"c\": {\"type\": \"null\"}}, \"required\": [\"b\"], "
        "\"additionalProperties\": false, \"title\": \"t\", \"description\": \"d\"}",
        "{\"anyOf\": [{\"type\": \"integer\"}, {\"$ref\": \"#/$defs/s\"}], \"$defs\": {\"s\": {\"type\": \"string\"}}}",
        "{\"oneOf\": [{\"type\": \"boolean\"}, {\"$ref\": \"#/definitions/n\"}], \"definitions\": {\"n\": {\"type\": \"null\"}}}",
        " \t\r\n{ \"type\" : \"object\" , \"properties\" : { } } \n"};
    int compiled = 0;
    for (const char* g : good) {
        for (int ws = 0; ws <= 1; ws++) {
            std::string pattern, error;
            EXPECT(json_schema_regex(g, std::strlen(g), ws, 1, pattern, error) == 0 && !pattern.empty() && error.empty());
            ByteDfa r;
            EXPECT(regex_compile(pattern.data(), pattern.size(), r, &at) == 0);
            compiled++;
        }
        // every truncation is refused as malformed JSON, with an offset inside the text (or at its end)
        const size_t n = std::strlen(g);
        size_t last = n;
        while (last > 0 && std::strchr(" \t\r\n", g[last - 1])) last--;
        for (size_t k = 0; k < last; k++) {
            std::string pattern, error;
            const std::string cut(g, k);                                                       // (its own buffer: a read past k is a finding)
            EXPECT(json_schema_regex(cut.data(), cut.size(), 0, 1, pattern, error) == kJsonSyntax && pattern.empty());
            EXPECT(!error.empty() && std::atoll(error.c_str()) >= 0 && std::atoll(error.c_str()) <= (long long)k);
        }
    }
    struct { const char* s; int code; const char* where; } bad[] = {
        {"{\"type\": \"integer\", \"minimum\": 1}", -4, "/minimum"},
        {"{\"type\": \"object\", \"properties\": {\"age\": {\"type\": \"integer\", \"maximum\": 9}}}", -4, "/properties/age/maximum"},
        {"{\"type\": \"string\", \"pattern\": \"a\"}", -4, "/pattern"}, {"{\"type\": \"string\", \"format\": \"date\"}", -4, "/format"},
        {"{\"type\": \"object\", \"additionalProperties\": true}", -4, "/additionalProperties"},
        {"{\"type\": \"object\", \"additionalProperties\": {}}", -4, "/additionalProperties"}, {"{\"patternProperties\": {}}", -4, "/patternProperties"},
        {"{\"allOf\": []}", -4, "/allOf"}, {"{\"not\": {}}", -4, "/not"}, {"{\"if\": {}}", -4, "/if"},
        {"{\"$ref\": \"#/$defs/a\", \"$defs\": {\"a\": {\"type\": \"array\", \"items\": {\"$ref\": \"#/$defs/a\"}}}}", -4, "/$ref/items/$ref"},
        {"{\"$ref\": \"#/$defs/b\"}", -4, "/$ref"}, {"{\"type\": \"string\", \"maxLength\": 256}", -4, "/maxLength"},
        {"{\"type\": \"array\", \"minItems\": 3, \"maxItems\": 2}", -4, "/maxItems"}, {"{\"type\": \"array\", \"minItems\": -1}", -4, "/minItems"},
        {"{\"enum\": [1.5]}", -4, "/enum/0"}, {"{\"enum\": [1, {}]}", -4, "/enum/1"}, {"{\"const\": []}", -4, "/const"}, {"{\"type\": \"float\"}", -4, "/type"},
        {"{\"type\": \"object\", \"properties\": {\"a\": {}}, \"required\": [\"z\"]}", -4, "/required"}, {"[]", -4, "/"}, {"3", -4, "/"},
        {"", -1, "0"}, {"{", -1, "1"}, {"{\"type\": }", -1, "9"}, {"{\"a\": 1,}", -1, "8"}, {"{\"a\": 01}", -1, "7"}, {"{\"a\": \"\\x\"}", -1, "8"},
        {"{\"a\": \"\\ud800\"}", -1, "13"}, {"{\"a\": tru}", -1, "9"}, {"{} x", -1, "3"}, {"{\"a\": \"\n\"}", -1, "7"}, {"{\"a\" 1}", -1, "5"}, {"{\"a\": 1.}", -1, "8"}};
    for (const auto& b : bad) {
        std::string pattern, error;
        const std::string own(b.s);
        const int rc = json_schema_regex(own.data(), own.size(), 0, 2, pattern, error);
        if (rc != b.code || error != b.where) std::printf("schema %s: %d at '%s', expected %d at '%s'\n", b.s, rc, error.c_str(), b.code, b.where);
        EXPECT(rc == b.code && error == b.where && pattern.empty());
    }
    {
        std::string deep, pattern, error;
        for (int k = 0; k < 70; k++) deep += "{\"a\": ";
        deep += "1";
        for (int k = 0; k < 70; k++) deep += "}";
        EXPECT(json_schema_regex(deep.data(), deep.size(), 0, 2, pattern, error) == kJsonSyntax);           // nesting above 64
        EXPECT(json_schema_regex("{}", 2, 2, 2, pattern, error) == kJsonSyntax && error.empty());
        EXPECT(json_schema_regex("{}", 2, 0, 5, pattern, error) == kJsonSyntax && error.empty());
        EXPECT(json_schema_regex(nullptr, 0, 0, 2, pattern, error) == kJsonSyntax);
        // 64 optional properties: the pattern stays small (quadratic), 65 are refused
        std::string props;
        for (int k = 0; k < 65; k++) {
            if (k == 64) {
                const std::string s = "{\"type\": \"object\", \"properties\": {" + props + "}}";
                EXPECT(json_schema_regex(s.data(), s.size(), 1, 2, pattern, error) == 0 && pattern.size() < 200000);
            }
            props += std::string(k ? ", " : "") + "\"k" + std::to_string(k) + "\": {\"type\": \"null\"}";
        }
        const std::string s = "{\"type\": \"object\", \"properties\": {" + props + "}}";
        EXPECT(json_schema_regex(s.data(), s.size(), 1, 2, pattern, error) == kJsonUnsupported && error == "/properties");
    }
    // a schema's pattern as a range of the pool
    {
        std::string pattern, error;
        const char* g = "{\"type\": \"object\", \"properties\": {\"a\": {\"type\": \"boolean\"}}, \"required\": [\"a\"]}";
        EXPECT(json_schema_regex(g, std::strlen(g), 0, 2, pattern, error) == 0);
        const int before = pool.n_states();
        EXPECT(pool.add_regex(pattern.data(), pattern.size(), 0, &at) == before && pool.n_states() > before);
        ByteDfa r;
        EXPECT(regex_compile(pattern.data(), pattern.size(), r, &at) == 0);
        EXPECT(regex_accepts(r, (const uint8_t*)"{\"a\":true}", 10) && !regex_accepts(r, (const uint8_t*)"{\"a\": true}", 11) && !regex_accepts(r, (const uint8_t*)"{}", 2));
        (void)pool.next();
    }
    if (failures) return 1;
    std::printf("host_text_automata ok (%d patterns, %d states)\n", compiled, pool.n_states());
    return 0;
}
