"""JSON schemas as patterns, restated in Python for the tests (include/gten_host_json.h, host/json_schema.h): the fixed
construction, character for character, and a validator of the same subset.  It runs none of the project's code."""
import json

STRING_HEAD = r'"(?:[^"\\\x00-\x1f]|\\["\\/bfnrt]|\\u[0-9a-fA-F]{4})'
INTEGER = r"-?(?:0|[1-9][0-9]{0,17})"
NUMBER = INTEGER + r"(?:\.[0-9]{1,17})?(?:[eE][+-]?[0-9]{1,3})?"
BOOLEAN = "(?:true|false)"
META = "\\.^$*+?()[]{}|"
KNOWN = {"type", "enum", "const", "properties", "required", "additionalProperties", "items", "minItems", "maxItems", "minLength", "maxLength", "anyOf",
         "oneOf", "$ref", "title", "description", "default", "examples", "$schema", "$id", "$defs", "definitions"}


class Refused(Exception):
    def __init__(self, path):
        super().__init__(path)
        self.path = path


def alt(v):
    return v[0] if len(v) == 1 else "(?:" + "|".join(v) + ")"


def literal_string(s):
    return "".join("\\" + c if c in META else c for c in json.dumps(s, ensure_ascii=False))


def any_value(depth, W):
    v = [STRING_HEAD + '*"', NUMBER, BOOLEAN, "null"]
    if depth > 0:
        A, S = any_value(depth - 1, W), STRING_HEAD + '*"'
        v.append(r"\[(?:" + A + "(?:," + W + A + r")*)?\]")
        v.append(r"\{(?:" + S + ":" + W + A + "(?:," + W + S + ":" + W + A + r")*)?\}")
    return alt(v)


class Compiler:
    def __init__(self, root, ws, depth):
        self.root, self.W, self.depth, self.refs = root, " ?" if ws else "", depth, []

    def bound(self, s, key, path):
        if key not in s:
            return None
        v = s[key]
        if isinstance(v, bool) or not isinstance(v, int) or v < 0 or v > 255:
            raise Refused(path + "/" + key)
        return v

    def literal(self, v, path):
        if isinstance(v, str):
            return literal_string(v)
        if v is True or v is False or v is None:
            return json.dumps(v)
        if isinstance(v, int):
            return str(v)
        raise Refused(path)

    def of_type(self, s, t, path):
        W = self.W
        if t == "string":
            m, M = self.bound(s, "minLength", path), self.bound(s, "maxLength", path)
            if M is not None and (m or 0) > M:
                raise Refused(path + "/maxLength")
            q = "*" if m is None and M is None else ("{%d,%d}" % (m or 0, M) if M is not None else "{%d,}" % m)
            return STRING_HEAD + q + '"'
        if t in ("integer", "number", "boolean", "null"):
            return {"integer": INTEGER, "number": NUMBER, "boolean": BOOLEAN, "null": "null"}[t]
        if t == "array":
            m, M = self.bound(s, "minItems", path) or 0, self.bound(s, "maxItems", path)
            if M is not None and m > M:
                raise Refused(path + "/maxItems")
            E = self.schema(s["items"], path + "/items") if "items" in s else any_value(max(self.depth - 1, 0), W)
            more = "(?:," + W + E + ")"
            if M == 0:
                return r"\[\]"
            if m == 0:
                return r"\[(?:" + E + more + ("*" if M is None else "{0,%d}" % (M - 1)) + r")?\]"
            return r"\[" + E + more + "{%d,%s}" % (m - 1, "" if M is None else M - 1) + r"\]"
        if t == "object":
            if "additionalProperties" in s and s["additionalProperties"] is not False:
                raise Refused(path + "/additionalProperties")
            props = s.get("properties", {})
            if not isinstance(props, dict) or len(props) > 64:
                raise Refused(path + "/properties")
            required = s.get("required", [])
            if not isinstance(required, list) or any(r not in props for r in required):
                raise Refused(path + "/required")
            kv = [(literal_string(k) + ":" + W + self.schema(v, path + "/properties/" + k), k in required) for k, v in props.items()]
            T = F = ""
            for p, req in reversed(kv):
                if req:
                    F, T = p + T, "," + W + p + T
                else:
                    F, T = "(?:" + p + T + "|" + F + ")", "(?:," + W + p + ")?" + T
            return r"\{" + F + r"\}"
        raise Refused(path + "/type")

    def schema(self, s, path):
        if not isinstance(s, dict):
            raise Refused(path)
        for k in s:
            if k not in KNOWN:
                raise Refused(path + "/" + k)
        if "$ref" in s:
            ref, target = s["$ref"], None
            for where in ("$defs", "definitions"):
                if isinstance(ref, str) and ref.startswith("#/" + where + "/"):
                    target = self.root.get(where, {}).get(ref[len(where) + 3:])
            if target is None or ref in self.refs:
                raise Refused(path + "/$ref")
            self.refs.append(ref)
            out = self.schema(target, path + "/$ref")
            self.refs.pop()
            return out
        if "const" in s:
            return self.literal(s["const"], path + "/const")
        if "enum" in s:
            if not isinstance(s["enum"], list) or not s["enum"]:
                raise Refused(path + "/enum")
            return alt([self.literal(v, path + "/enum/%d" % k) for k, v in enumerate(s["enum"])])
        for key in ("anyOf", "oneOf"):
            if key in s:
                if not isinstance(s[key], list) or not s[key]:
                    raise Refused(path + "/" + key)
                return alt([self.schema(v, path + "/%s/%d" % (key, k)) for k, v in enumerate(s[key])])
        if "type" not in s:
            return any_value(self.depth, self.W)
        t = s["type"]
        if isinstance(t, str):
            return self.of_type(s, t, path)
        if not isinstance(t, list) or not t or not all(isinstance(x, str) for x in t):
            raise Refused(path + "/type")
        return alt([self.of_type(s, x, path) for x in t])


def regex(schema, ws=0, depth=2):
    return Compiler(schema, ws, depth).schema(schema, "")


def valid(schema, doc, root=None, depth=2):
    """whether the parsed document fits the schema, for the subset above (objects: exactly the listed keys, in the listed order)"""
    root = schema if root is None else root
    s = schema
    if "$ref" in s:
        return valid(root[s["$ref"].split("/")[1]][s["$ref"].split("/")[2]], doc, root, depth)
    same = lambda a, b: type(a) is type(b) and a == b      # noqa: E731  (True is not 1)
    if "const" in s:
        return same(s["const"], doc)
    if "enum" in s:
        return any(same(v, doc) for v in s["enum"])
    for key in ("anyOf", "oneOf"):
        if key in s:
            return any(valid(v, doc, root, depth) for v in s[key])
    if "type" not in s:
        return nesting(doc) <= depth
    types = [s["type"]] if isinstance(s["type"], str) else s["type"]
    return any(valid_type(s, t, doc, root, depth) for t in types)


def nesting(doc):
    if isinstance(doc, list):
        return 1 + max([nesting(v) for v in doc] + [0])
    if isinstance(doc, dict):
        return 1 + max([nesting(v) for v in doc.values()] + [0])
    return 0


def valid_type(s, t, doc, root, depth):
    if t == "string":
        return isinstance(doc, str) and s.get("minLength", 0) <= len(doc) <= s.get("maxLength", len(doc))
    if t == "integer":
        return isinstance(doc, int) and not isinstance(doc, bool)
    if t == "number":
        return isinstance(doc, (int, float)) and not isinstance(doc, bool)
    if t == "boolean":
        return isinstance(doc, bool)
    if t == "null":
        return doc is None
    if t == "array":
        if not isinstance(doc, list) or not s.get("minItems", 0) <= len(doc) <= s.get("maxItems", len(doc)):
            return False
        return all(valid(s["items"], v, root, depth) if "items" in s else nesting(v) <= max(depth - 1, 0) for v in doc)
    if t == "object":
        props = s.get("properties", {})
        if not isinstance(doc, dict) or any(k not in props for k in doc) or any(r not in doc for r in s.get("required", [])):
            return False
        return list(doc) == [k for k in props if k in doc] and all(valid(props[k], v, root, depth) for k, v in doc.items())
    return False
