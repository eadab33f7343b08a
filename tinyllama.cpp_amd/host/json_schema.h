// json_schema.h -- a subset of JSON Schema compiled to a pattern of the regex dialect of host/regex_build.h.  Host
// C++ with no device call.  The pattern is a string of that dialect and nothing else: add_regex() of it is the whole of "emit JSON
// that fits this schema", so the expansion over the vocabulary runs on the device and ending follows the regex rule.
//
// json_parse(): a small JSON reader -- objects (member order kept), arrays, strings with every escape, numbers, true / false / null;
// nesting up to kJsonMaxDepth; a malformed text is refused with the byte offset of the offence.
//
// json_schema_regex(): the construction is FIXED, so that a restatement gives the same string character for character.  W is empty
// for ws = 0 and " ?" for ws = 1, placed after every `,` and `:` and nowhere else.  alt(a, b, ..) is a alone, or (?:a|b|..).
//   string    "(?:[^"\\\x00-\x1f]|\\["\\/bfnrt]|\\u[0-9a-fA-F]{4})*"      minLength / maxLength replace * by {m,n} / {m,}
//   integer   -?(?:0|[1-9][0-9]{0,17})
//   number    integer, then (?:\.[0-9]{1,17})?(?:[eE][+-]?[0-9]{1,3})?
//   boolean   (?:true|false)          null   null
//   enum / const: alt of the values in order -- a string as its compact JSON text (what Python's json.dumps(v, ensure_ascii=False)
//             gives) with every one of  \ . ^ $ * + ? ( ) [ ] { } |  escaped by a backslash; an integer as its decimal text; true, false, null
//   array     E the element (items; absent: any value one level down), m = minItems (0), M = maxItems (unbounded):
//             M == 0: \[\]      m == 0: \[(?:E(?:,WE){0,M-1})?\]      else: \[E(?:,WE){m-1,M-1}\]      unbounded M: * and {m-1,}
//   object    properties in the order of `properties`, K the key as an enum string, P = (started ? ",W" : "") K:WV; the body is
//             R(1, false) with R(i, started) = "" behind the last property; a required property gives P R(i+1, true); an optional one
//             gives (?:P R(i+1, true)|R(i+1, false)) while nothing has started, and (?:P)?R(i+1, true) once something has -- the same
//             language as (?:P R(i+1, true)|R(i+1, true)) without writing R(i+1, true) twice, which would double the pattern per
//             optional property; as it is the pattern is quadratic in the number of properties.  The whole is \{ body \}.
//   no type   any JSON value of up to `depth` levels of nesting: level 0 is alt(string, number, boolean, null); level d adds
//             \[(?:A(?:,WA)*)?\] and \{(?:S:WA(?:,WS:WA)*)?\} with A the level below and S the string pattern
//   type as a list, anyOf, oneOf: alt in order.  $ref to #/$defs/NAME or #/definitions/NAME: expanded in place.
//   ignored: title description default examples $schema $id $defs definitions
// Refused with kJsonUnsupported (-4) and the offending key's path ("/properties/age/minimum"): every other key, additionalProperties
// other than false, a recursive or unresolvable $ref, a bound above 255 or not a non-negative integer, minimum above maximum, enum values
// that are objects, arrays or non-integers, a `required` name that is no property, more than kJsonMaxProperties properties, a schema
// that is no object.  kJsonSyntax (-1) with the byte offset as decimal text: malformed JSON.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace gten {

enum : int { kJsonSyntax = -1, kJsonUnsupported = -4 };
constexpr int kJsonMaxDepth = 64;
constexpr int kJsonMaxProperties = 64;
constexpr int kJsonMaxBound = 255;
constexpr int kJsonMaxAnyDepth = 4;

struct JsonValue {
    enum Kind { Null, Bool, Number, String, Array, Object } kind = Null;
    bool b = false;
    std::string s;                                          // String: its bytes (UTF-8); Number: its text
    std::vector<JsonValue> items;                           // Array
    std::vector<std::pair<std::string, JsonValue>> members; // Object, in the text's order
    const JsonValue* get(const char* key) const
    {
        if (kind != Object) return nullptr;
        for (const auto& m : members)
            if (m.first == key) return &m.second;
        return nullptr;
    }
    bool is_integer() const { return kind == Number && s.find_first_of(".eE") == std::string::npos; }
};

namespace json_detail {

struct Reader {
    const char* p;
    size_t n, at = 0;
    size_t err = 0;
    bool fail(size_t where) { err = where; return false; }
    void skip()
    {
        while (at < n && (p[at] == ' ' || p[at] == '\t' || p[at] == '\n' || p[at] == '\r')) at++;
    }
    static void utf8(unsigned cp, std::string& out)
    {
        if (cp < 0x80) out += (char)cp;
        else if (cp < 0x800) { out += (char)(0xC0 | (cp >> 6)); out += (char)(0x80 | (cp & 0x3F)); }
        else if (cp < 0x10000) { out += (char)(0xE0 | (cp >> 12)); out += (char)(0x80 | ((cp >> 6) & 0x3F)); out += (char)(0x80 | (cp & 0x3F)); }
        else { out += (char)(0xF0 | (cp >> 18)); out += (char)(0x80 | ((cp >> 12) & 0x3F)); out += (char)(0x80 | ((cp >> 6) & 0x3F)); out += (char)(0x80 | (cp & 0x3F)); }
    }
    bool hex4(unsigned& v)
    {
        if (at + 4 > n) return fail(n);
        v = 0;
        for (int k = 0; k < 4; k++) {
            const char c = p[at + (size_t)k];
            int d;
            if (c >= '0' && c <= '9') d = c - '0';
            else if (c >= 'a' && c <= 'f') d = c - 'a' + 10;
            else if (c >= 'A' && c <= 'F') d = c - 'A' + 10;
            else return fail(at + (size_t)k);
            v = v * 16 + (unsigned)d;
        }
        at += 4;
        return true;
    }
    bool string(std::string& out)
    {
        if (at >= n || p[at] != '"') return fail(at);
        at++;
        for (;;) {
            if (at >= n) return fail(n);
            const unsigned char c = (unsigned char)p[at];
            if (c == '"') { at++; return true; }
            if (c < 0x20) return fail(at);
            if (c != '\\') { out += (char)c; at++; continue; }
            if (at + 1 >= n) return fail(n);
            const char e = p[at + 1];
            at += 2;
            switch (e) {
            case '"': out += '"'; break;
            case '\\': out += '\\'; break;
            case '/': out += '/'; break;
            case 'b': out += '\b'; break;
            case 'f': out += '\f'; break;
            case 'n': out += '\n'; break;
            case 'r': out += '\r'; break;
            case 't': out += '\t'; break;
            case 'u': {
                unsigned cp = 0;
                if (!hex4(cp)) return false;
                if (cp >= 0xD800 && cp < 0xDC00) {                     // a high surrogate needs its low one
                    unsigned lo = 0;
                    if (at + 2 > n || p[at] != '\\' || p[at + 1] != 'u') return fail(at < n ? at : n);
                    at += 2;
                    if (!hex4(lo)) return false;
                    if (lo < 0xDC00 || lo > 0xDFFF) return fail(at - 4);
                    cp = 0x10000 + ((cp - 0xD800) << 10) + (lo - 0xDC00);
                } else if (cp >= 0xDC00 && cp < 0xE000) {
                    return fail(at - 4);
                }
                utf8(cp, out);
                break;
            }
            default: return fail(at - 1);
            }
        }
    }
    bool digits()
    {
        const size_t from = at;
        while (at < n && p[at] >= '0' && p[at] <= '9') at++;
        return at > from ? true : fail(at);
    }
    bool number(JsonValue& v)
    {
        const size_t from = at;
        if (at < n && p[at] == '-') at++;
        if (at < n && p[at] == '0') at++;
        else if (!digits()) return false;
        if (at < n && p[at] == '.') { at++; if (!digits()) return false; }
        if (at < n && (p[at] == 'e' || p[at] == 'E')) {
            at++;
            if (at < n && (p[at] == '+' || p[at] == '-')) at++;
            if (!digits()) return false;
        }
        v.kind = JsonValue::Number;
        v.s.assign(p + from, at - from);
        return true;
    }
    bool literal(const char* word)
    {
        const size_t m = std::strlen(word);
        for (size_t k = 0; k < m; k++)
            if (at + k >= n || p[at + k] != word[k]) return fail(at + k < n ? at + k : n);
        at += m;
        return true;
    }
    bool value(JsonValue& v, int depth)
    {
        skip();
        if (at >= n) return fail(n);
        if (depth > kJsonMaxDepth) return fail(at);
        const char c = p[at];
        if (c == '{') {
            v.kind = JsonValue::Object;
            at++;
            skip();
            if (at < n && p[at] == '}') { at++; return true; }
            for (;;) {
                skip();
                std::string key;
                if (!string(key)) return false;
                skip();
                if (at >= n || p[at] != ':') return fail(at < n ? at : n);
                at++;
                v.members.emplace_back(std::move(key), JsonValue{});
                if (!value(v.members.back().second, depth + 1)) return false;
                skip();
                if (at < n && p[at] == ',') { at++; continue; }
                if (at < n && p[at] == '}') { at++; return true; }
                return fail(at < n ? at : n);
            }
        }
        if (c == '[') {
            v.kind = JsonValue::Array;
            at++;
            skip();
            if (at < n && p[at] == ']') { at++; return true; }
            for (;;) {
                v.items.emplace_back();
                if (!value(v.items.back(), depth + 1)) return false;
                skip();
                if (at < n && p[at] == ',') { at++; continue; }
                if (at < n && p[at] == ']') { at++; return true; }
                return fail(at < n ? at : n);
            }
        }
        if (c == '"') { v.kind = JsonValue::String; return string(v.s); }
        if (c == 't') { v.kind = JsonValue::Bool; v.b = true; return literal("true"); }
        if (c == 'f') { v.kind = JsonValue::Bool; v.b = false; return literal("false"); }
        if (c == 'n') { v.kind = JsonValue::Null; return literal("null"); }
        if (c == '-' || (c >= '0' && c <= '9')) return number(v);
        return fail(at);
    }
};

} // namespace json_detail

// the n bytes of text as one JSON value: 0, or kJsonSyntax with *error_offset (may be NULL) the byte offset of the offence
inline int json_parse(const char* text, size_t n, JsonValue& out, long long* error_offset)
{
    if (error_offset) *error_offset = -1;
    json_detail::Reader r{text, n};
    out = JsonValue{};
    bool ok = text && r.value(out, 0);
    if (ok) {
        r.skip();
        if (r.at != n) ok = r.fail(r.at);
    }
    if (!ok && error_offset) *error_offset = (long long)r.err;
    return ok ? 0 : kJsonSyntax;
}

namespace json_detail {

inline std::string alt(const std::vector<std::string>& v)
{
    if (v.size() == 1) return v[0];
    std::string out = "(?:";
    for (size_t k = 0; k < v.size(); k++) out += (k ? "|" : "") + v[k];
    return out + ")";
}

// the string as compact JSON text (json.dumps(s, ensure_ascii=False)) with the dialect's metacharacters escaped
inline std::string literal_string(const std::string& s)
{
    std::string js = "\"";
    for (const char ch : s) {
        const unsigned char c = (unsigned char)ch;
        switch (c) {
        case '"': js += "\\\""; break;
        case '\\': js += "\\\\"; break;
        case '\n': js += "\\n"; break;
        case '\r': js += "\\r"; break;
        case '\t': js += "\\t"; break;
        case '\b': js += "\\b"; break;
        case '\f': js += "\\f"; break;
        default:
            if (c < 0x20) {
                char buf[8];
                std::snprintf(buf, sizeof buf, "\\u%04x", (unsigned)c);
                js += buf;
            } else {
                js += ch;
            }
        }
    }
    js += '"';
    std::string out;
    for (const char c : js) {
        if (std::strchr("\\.^$*+?()[]{}|", c) && c != 0) out += '\\';
        out += c;
    }
    return out;
}

struct Compiler {
    const JsonValue* root;
    std::string W;
    int any_depth;
    std::string err_path;
    std::vector<std::string> ref_stack;

    static const char* kString() { return "\"(?:[^\"\\\\\\x00-\\x1f]|\\\\[\"\\\\/bfnrt]|\\\\u[0-9a-fA-F]{4})"; }   // (the quantifier and the closing quote follow)
    static const char* kInteger() { return "-?(?:0|[1-9][0-9]{0,17})"; }
    static std::string number() { return std::string(kInteger()) + "(?:\\.[0-9]{1,17})?(?:[eE][+-]?[0-9]{1,3})?"; }
    static std::string string_any() { return std::string(kString()) + "*\""; }

    bool refuse(const std::string& path) { err_path = path; return false; }

    // a bound: a non-negative integer of at most kJsonMaxBound
    bool bound(const JsonValue& s, const char* key, const std::string& path, int& out, bool& present)
    {
        const JsonValue* v = s.get(key);
        present = v != nullptr;
        if (!v) return true;
        if (!v->is_integer() || v->s.size() > 3 || v->s[0] == '-') return refuse(path + "/" + key);
        out = std::atoi(v->s.c_str());
        return out <= kJsonMaxBound ? true : refuse(path + "/" + key);
    }

    std::string any(int depth) const
    {
        std::vector<std::string> v{string_any(), number(), "(?:true|false)", "null"};
        if (depth > 0) {
            const std::string A = any(depth - 1), S = string_any();
            v.push_back("\\[(?:" + A + "(?:," + W + A + ")*)?\\]");
            v.push_back("\\{(?:" + S + ":" + W + A + "(?:," + W + S + ":" + W + A + ")*)?\\}");
        }
        return alt(v);
    }

    bool value_literal(const JsonValue& v, const std::string& path, std::string& out)
    {
        switch (v.kind) {
        case JsonValue::String: out = literal_string(v.s); return true;
        case JsonValue::Bool: out = v.b ? "true" : "false"; return true;
        case JsonValue::Null: out = "null"; return true;
        case JsonValue::Number:
            if (!v.is_integer()) return refuse(path);
            out = v.s == "-0" ? "0" : v.s;
            return true;
        default: return refuse(path);
        }
    }

    bool of_type(const JsonValue& s, const std::string& type, const std::string& path, std::string& out)
    {
        if (type == "string") {
            int m = 0, M = 0;
            bool has_m = false, has_M = false;
            if (!bound(s, "minLength", path, m, has_m) || !bound(s, "maxLength", path, M, has_M)) return false;
            if (has_M && m > M) return refuse(path + "/maxLength");
            std::string q = "*";
            if (has_M) q = "{" + std::to_string(m) + "," + std::to_string(M) + "}";
            else if (has_m) q = "{" + std::to_string(m) + ",}";
            out = std::string(kString()) + q + "\"";
            return true;
        }
        if (type == "integer") { out = kInteger(); return true; }
        if (type == "number") { out = number(); return true; }
        if (type == "boolean") { out = "(?:true|false)"; return true; }
        if (type == "null") { out = "null"; return true; }
        if (type == "array") {
            int m = 0, M = 0;
            bool has_m = false, has_M = false;
            if (!bound(s, "minItems", path, m, has_m) || !bound(s, "maxItems", path, M, has_M)) return false;
            if (has_M && m > M) return refuse(path + "/maxItems");
            std::string E;
            if (const JsonValue* items = s.get("items")) {
                if (!schema(*items, path + "/items", E)) return false;
            } else {
                E = any(any_depth > 0 ? any_depth - 1 : 0);
            }
            const std::string more = "(?:," + W + E + ")";
            if (has_M && M == 0) out = "\\[\\]";
            else if (m == 0) out = "\\[(?:" + E + more + (has_M ? "{0," + std::to_string(M - 1) + "}" : std::string("*")) + ")?\\]";
            else out = "\\[" + E + more + "{" + std::to_string(m - 1) + "," + (has_M ? std::to_string(M - 1) : std::string()) + "}\\]";
            return true;
        }
        if (type == "object") {
            if (const JsonValue* ap = s.get("additionalProperties"))
                if (ap->kind != JsonValue::Bool || ap->b) return refuse(path + "/additionalProperties");
            const JsonValue* props = s.get("properties");
            if (props && props->kind != JsonValue::Object) return refuse(path + "/properties");
            const size_t n = props ? props->members.size() : 0;
            if (n > (size_t)kJsonMaxProperties) return refuse(path + "/properties");
            std::vector<char> required(n, 0);
            if (const JsonValue* req = s.get("required")) {
                if (req->kind != JsonValue::Array) return refuse(path + "/required");
                for (const JsonValue& r : req->items) {
                    size_t k = 0;
                    while (r.kind == JsonValue::String && k < n && props->members[k].first != r.s) k++;
                    if (r.kind != JsonValue::String || k == n) return refuse(path + "/required");
                    required[k] = 1;
                }
            }
            std::vector<std::string> kv(n);
            for (size_t i = 0; i < n; i++) {
                std::string V;
                if (!schema(props->members[i].second, path + "/properties/" + props->members[i].first, V)) return false;
                kv[i] = literal_string(props->members[i].first) + ":" + W + V;
            }
            // R(i, started) from the last property backwards: T = R(i, true), F = R(i, false)
            std::string T, F;
            for (size_t i = n; i-- > 0;) {
                const std::string Pt = "," + W + kv[i], Pf = kv[i];
                if (required[i]) { F = Pf + T; T = Pt + T; }
                else { F = "(?:" + Pf + T + "|" + F + ")"; T = "(?:" + Pt + ")?" + T; }
            }
            out = "\\{" + F + "\\}";
            return true;
        }
        return refuse(path + "/type");
    }

    bool resolve(const std::string& ref, const std::string& path, std::string& out)
    {
        const JsonValue* target = nullptr;
        for (const char* where : {"$defs", "definitions"}) {
            const std::string prefix = std::string("#/") + where + "/";
            if (ref.compare(0, prefix.size(), prefix) != 0) continue;
            const JsonValue* defs = root->get(where);
            if (defs) target = defs->get(ref.c_str() + prefix.size());
        }
        if (!target) return refuse(path + "/$ref");
        for (const std::string& r : ref_stack)
            if (r == ref) return refuse(path + "/$ref");                               // (recursive)
        ref_stack.push_back(ref);
        const bool ok = schema(*target, path + "/$ref", out);
        ref_stack.pop_back();
        return ok;
    }

    bool schema(const JsonValue& s, const std::string& path, std::string& out)
    {
        if (s.kind != JsonValue::Object) return refuse(path);
        static const char* const known[] = {"type", "enum", "const", "properties", "required", "additionalProperties", "items", "minItems", "maxItems", "minLength",
                                            "maxLength", "anyOf", "oneOf", "$ref", "title", "description", "default", "examples", "$schema", "$id", "$defs",
                                            "definitions"};
        for (const auto& m : s.members) {
            bool ok = false;
            for (const char* k : known) ok |= m.first == k;
            if (!ok) return refuse(path + "/" + m.first);
        }
        if (const JsonValue* ref = s.get("$ref")) {
            if (ref->kind != JsonValue::String) return refuse(path + "/$ref");
            return resolve(ref->s, path, out);
        }
        if (const JsonValue* c = s.get("const")) return value_literal(*c, path + "/const", out);
        if (const JsonValue* e = s.get("enum")) {
            if (e->kind != JsonValue::Array || e->items.empty()) return refuse(path + "/enum");
            std::vector<std::string> v(e->items.size());
            for (size_t k = 0; k < v.size(); k++)
                if (!value_literal(e->items[k], path + "/enum/" + std::to_string(k), v[k])) return false;
            out = alt(v);
            return true;
        }
        for (const char* key : {"anyOf", "oneOf"})
            if (const JsonValue* a = s.get(key)) {
                if (a->kind != JsonValue::Array || a->items.empty()) return refuse(path + "/" + key);
                std::vector<std::string> v(a->items.size());
                for (size_t k = 0; k < v.size(); k++)
                    if (!schema(a->items[k], path + "/" + key + "/" + std::to_string(k), v[k])) return false;
                out = alt(v);
                return true;
            }
        const JsonValue* type = s.get("type");
        if (!type) { out = any(any_depth); return true; }
        if (type->kind == JsonValue::String) return of_type(s, type->s, path, out);
        if (type->kind != JsonValue::Array || type->items.empty()) return refuse(path + "/type");
        std::vector<std::string> v(type->items.size());
        for (size_t k = 0; k < v.size(); k++)
            if (type->items[k].kind != JsonValue::String || !of_type(s, type->items[k].s, path, v[k])) return err_path.empty() ? refuse(path + "/type") : false;
        out = alt(v);
        return true;
    }
};

} // namespace json_detail

// The schema (n bytes of JSON) as a pattern: 0 with `pattern`, or kJsonSyntax / kJsonUnsupported with `error` the byte offset as
// decimal text / the offending key's path.  ws 0 or 1; depth 0 .. kJsonMaxAnyDepth (bad values: kJsonSyntax with an empty error).
inline int json_schema_regex(const char* schema, size_t n, int ws, int depth, std::string& pattern, std::string& error)
{
    pattern.clear();
    error.clear();
    if (!schema || ws < 0 || ws > 1 || depth < 0 || depth > kJsonMaxAnyDepth) return kJsonSyntax;
    JsonValue root;
    long long off = -1;
    if (json_parse(schema, n, root, &off)) {
        error = std::to_string(off);
        return kJsonSyntax;
    }
    json_detail::Compiler c{&root, ws ? " ?" : "", depth, {}, {}};
    if (!c.schema(root, "", pattern)) {
        pattern.clear();
        error = c.err_path.empty() ? "/" : c.err_path;
        return kJsonUnsupported;
    }
    return 0;
}

} // namespace gten
