"""not gpu: JSON schemas compiled to the regex dialect (include/gten_host_json.h, host/json_schema.h).  The pattern is
held to the restatement of tests/json_schema_ref.py character for character; to Python's re on documents json.dumps makes from
instances that fit and on near misses; its byte automaton to json.loads and a validator of the subset on strings sampled from it; and
every refusal to its path or offset."""
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import json_schema_ref as ref  # noqa: E402
import regex_ref  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402


@pytest.fixture(scope="module")
def libs():
    pkg = load_package()
    pkg.build.build_all()
    return pkg, pkg.hostabi.GtenHost()


class Raw(str):
    """a near miss given as text, not as a document for json.dumps"""


PERSON = {"type": "object", "title": "person", "description": "ignored", "additionalProperties": False,
          "properties": {"nick": {"type": "string", "maxLength": 8}, "name": {"type": "string", "minLength": 1}, "age": {"type": "integer"},
                         "tags": {"type": "array", "items": {"enum": ["a.b", "c|d", "e\"f\\g", "é"]}, "maxItems": 3},
                         "score": {"type": ["number", "null"]}, "ok": {"type": "boolean"}},
          "required": ["name", "score"]}
# (schema, documents that fit, documents that do not -- as texts where the fault is one of form)
CASES = [
    ({"type": "string"}, ["", "a", "é\n\"\\\u0001😀"], [3, None]),
    ({"type": "string", "minLength": 2, "maxLength": 4}, ["ab", "abcd", "é\n"], ["a", "abcde"]),
    ({"type": "string", "minLength": 3}, ["abc", "abcdefgh"], ["ab"]),
    ({"type": "string", "maxLength": 2}, ["", "ab"], ["abc"]),
    ({"type": "integer"}, [0, -1, 7, 10 ** 17], [1.5, "1", Raw("01"), Raw("-01"), Raw("+1"), Raw("1.0")]),
    ({"type": "number"}, [0, -1.5, 3.25, 1e-5, 2.5e20], [Raw("1."), Raw(".5"), Raw("1e"), Raw("01.5"), "x"]),
    ({"type": "boolean"}, [True, False], [None, 0]),
    ({"type": "null"}, [None], [False]),
    ({"type": ["integer", "string", "null"]}, [1, "x", None], [True, 1.5]),
    ({"enum": ["a.b", 3, -7, True, None, "x y", "(*)"]}, ["a.b", 3, -7, True, None, "x y", "(*)"], ["aXb", 4, False, "x  y"]),
    ({"const": "only{this}"}, ["only{this}"], ["only"]),
    ({"const": 12}, [12], [1, 122]),
    ({"type": "array", "items": {"type": "integer"}}, [[], [1], [1, 2, 3, 4, 5]], [[1, "a"], Raw("[1,]"), Raw("[,1]"), Raw("[1 ,2]")]),                    # m 0, M unbounded
    ({"type": "array", "items": {"type": "integer"}, "maxItems": 2}, [[], [1], [1, 2]], [[1, 2, 3]]),                            # m 0, M bounded
    ({"type": "array", "items": {"type": "boolean"}, "minItems": 2}, [[True, False], [True] * 5], [[], [True]]),                 # m > 0, M unbounded
    ({"type": "array", "items": {"type": "null"}, "minItems": 1, "maxItems": 3}, [[None], [None] * 3], [[], [None] * 4]),         # m > 0, M bounded
    ({"type": "array", "maxItems": 0}, [[]], [[1]]),
    ({"type": "array", "items": {"type": "integer"}, "minItems": 1, "maxItems": 1}, [[4]], [[], [4, 4]]),
    ({"type": "array"}, [[], [1, "a", None, [2], {"k": 1}]], [[[[1]]]]),                                                         # any value one level down
    (PERSON, [{"name": "x", "score": None}, {"nick": "n", "name": "x", "age": 3, "tags": ["a.b", "é"], "score": 1.5, "ok": True},
              {"name": "x", "tags": [], "score": 2}, {"name": "x", "score": 0, "ok": False}, {"name": "y", "age": 1, "score": -1}],
     [{"name": "x"}, {"age": 1, "name": "y", "score": -1}, {"name": "x", "score": 1, "extra": 1}, Raw('{"score":1,"name":"x"}'), Raw('{"name":"x","score":1,}'), Raw('{"name":"x","age":03,"score":1}'),
      Raw('{"name":"x\ny","score":1}'), {"name": "", "score": 1}, {"name": "x", "score": 1, "tags": ["zz"]}, Raw('{"name":"x" ,"score":1}')]),
    ({"type": "object", "properties": {"a": {"type": "integer"}, "b": {"type": "integer"}, "c": {"type": "integer"}}, "required": ["b", "c"]},    # optional first
     [{"b": 1, "c": 2}, {"a": 0, "b": 1, "c": 2}], [{"a": 0, "c": 2}, {}]),
    ({"type": "object", "properties": {"a": {"type": "integer"}, "b": {"type": "integer"}, "c": {"type": "integer"}}, "required": ["a", "b"]},    # optional last
     [{"a": 0, "b": 1}, {"a": 0, "b": 1, "c": 2}], [{"a": 0, "c": 2}]),
    ({"type": "object", "properties": {"a": {"type": "integer"}, "b": {"type": "integer"}, "c": {"type": "integer"}}, "required": ["a", "c"]},    # optional in the middle
     [{"a": 0, "c": 2}, {"a": 0, "b": 1, "c": 2}], [{"a": 0, "b": 1}]),
    ({"type": "object", "properties": {"a": {"type": "integer"}, "b": {"type": "integer"}, "c": {"type": "integer"}}},                              # all optional
     [{}, {"a": 0}, {"b": 1}, {"c": 2}, {"a": 0, "c": 2}, {"b": 1, "c": 2}, {"a": 0, "b": 1, "c": 2}], [Raw('{,"a":0}'), Raw('{"a":0,}'), Raw('{"c":2,"a":0}')]),
    ({"type": "object"}, [{}], [{"a": 1}]),
    ({"anyOf": [{"type": "integer"}, {"$ref": "#/$defs/pair"}], "$defs": {"pair": {"type": "array", "items": {"$ref": "#/$defs/leaf"}, "minItems": 2, "maxItems": 2},
                                                                           "leaf": {"type": "string"}}}, [3, ["a", "b"]], [["a"], "a"]),
    ({"oneOf": [{"type": "null"}, {"$ref": "#/definitions/flag"}], "definitions": {"flag": {"type": "boolean"}}, "$schema": "x", "$id": "y", "default": 1,
      "examples": [1]}, [None, True], [0]),
    ({}, [1, "a", None, True, [1, [2]], {"k": {"j": 1}}, {"k": [1, "x"], "l": {}}], [[[[1]]], {"k": [1, {"j": []}]}, {"a": {"b": {"c": 1}}}]),                                 # depth 2
]
IDS = [str(k) for k in range(len(CASES))]


@pytest.mark.parametrize("case", CASES, ids=IDS)
@pytest.mark.parametrize("ws", [0, 1])
def test_the_pattern_is_the_restatements_and_pythons_re_agrees(libs, case, ws):
    pkg, host = libs
    schema, fits, misses = case
    pattern = host.json_schema_regex(schema, ws)
    assert pattern == ref.regex(schema, ws)
    assert host.json_schema_regex(json.dumps(schema), ws) == pattern       # a dict or its text
    n256, acc = pkg.hostabi.byte_dfa(host, pattern)                                     # the dialect takes it
    print(f"schema {json.dumps(schema)[:60]} ws {ws}: pattern of {len(pattern)} characters, {len(acc)} byte states")
    styles = [dict(separators=(",", ":")), {}] if ws else [dict(separators=(",", ":"))]
    for doc in fits:
        assert ref.valid(schema, doc), doc
        for style in styles:
            text = json.dumps(doc, ensure_ascii=False, **style)
            assert re.fullmatch(pattern, text, re.ASCII) is not None, (text, pattern)
            assert regex_ref.accepts(n256, acc, text.encode()), text
    for doc in misses:
        text = str(doc) if isinstance(doc, Raw) else json.dumps(doc, ensure_ascii=False, separators=(",", ":"))
        assert re.fullmatch(pattern, text, re.ASCII) is None, (text, pattern)
        assert not regex_ref.accepts(n256, acc, text.encode()), text
    for doc in fits:                                                       # ws = 0 takes the compact style only
        spaced, compact = json.dumps(doc, ensure_ascii=False), json.dumps(doc, ensure_ascii=False, separators=(",", ":"))
        if not ws and spaced != compact and not isinstance(doc, str):
            assert re.fullmatch(pattern, spaced, re.ASCII) is None, spaced


def test_depth_bounds_the_nesting_of_any_value(libs):
    pkg, host = libs
    docs = [1, [1], [[1]], [[[1]]], [[[[1]]]], {"a": [{"b": [1]}]}]
    for depth in range(5):
        pattern = host.json_schema_regex({}, 0, depth)
        assert pattern == ref.regex({}, 0, depth)
        for doc in docs:
            text = json.dumps(doc, separators=(",", ":"))
            assert (re.fullmatch(pattern, text, re.ASCII) is not None) == (ref.nesting(doc) <= depth), (depth, text)
    # an array without items inside a typed schema holds any value one level below `depth`
    assert host.json_schema_regex({"type": "array"}, 0, 3) == ref.regex({"type": "array"}, 0, 3)


def sample(n256, acc, g, max_len=400):
    """a random walk over the byte automaton that ends at an accepting state: at each state one of the live bytes, stopping with
    probability 1/3 where it may; None when it runs too long"""
    s, out = 0, bytearray()
    while len(out) < max_len:
        if acc[s] and (g.integers(0, 3) == 0 or not (n256[s] != regex_ref.NONE).any()):
            return bytes(out)
        live = np.flatnonzero(n256[s] != regex_ref.NONE)
        # prefer the bytes that close something, so that walks end
        closing = [b for b in live if b in b'"}],' or 0x30 <= b <= 0x39]
        b = int(g.choice(closing if closing and g.integers(0, 2) else live))
        out.append(b)
        s = int(n256[s][b])
    return None


@pytest.mark.parametrize("k", [0, 4, 5, 9, 13, 15, 19, 23, 25, 27], ids=str)
def test_strings_sampled_from_the_automaton_are_json_that_fits(libs, k):
    pkg, host = libs
    schema = CASES[k][0]
    g = np.random.default_rng(100 + k)
    for ws in (0, 1):
        n256, acc = pkg.hostabi.byte_dfa(host, host.json_schema_regex(schema, ws, 1))
        done = 0
        for _ in range(60):
            raw = sample(n256, acc, g)
            if raw is None:
                continue
            doc = json.loads(raw.decode("utf-8"))                          # every accepted string is UTF-8 and JSON
            assert ref.valid(schema, doc, depth=1), (raw, schema)
            done += 1
        assert done >= 20, done


REFUSED = [
    ({"type": "integer", "minimum": 1}, "/minimum"), ({"type": "integer", "maximum": 1}, "/maximum"),
    ({"type": "object", "properties": {"age": {"type": "integer", "minimum": 0}}}, "/properties/age/minimum"),
    ({"type": "string", "pattern": "a+"}, "/pattern"), ({"type": "string", "format": "date"}, "/format"),
    ({"type": "object", "additionalProperties": True}, "/additionalProperties"), ({"type": "object", "additionalProperties": {"type": "string"}}, "/additionalProperties"),
    ({"type": "object", "patternProperties": {}}, "/patternProperties"), ({"allOf": [{}]}, "/allOf"), ({"not": {}}, "/not"), ({"if": {}}, "/if"),
    ({"$ref": "#/$defs/a", "$defs": {"a": {"type": "array", "items": {"$ref": "#/$defs/a"}}}}, "/$ref/items/$ref"),                # recursive
    ({"$ref": "#/$defs/missing"}, "/$ref"), ({"$ref": "http://x/y"}, "/$ref"),
    ({"type": "string", "maxLength": 256}, "/maxLength"), ({"type": "array", "minItems": 256}, "/minItems"),
    ({"type": "array", "items": {"type": "array", "maxItems": 1000}}, "/items/maxItems"), ({"type": "array", "minItems": 3, "maxItems": 2}, "/maxItems"),
    ({"enum": [1.5]}, "/enum/0"), ({"enum": ["a", {"b": 1}]}, "/enum/1"), ({"enum": [[1]]}, "/enum/0"), ({"const": 2.5}, "/const"), ({"enum": []}, "/enum"),
    ({"type": "float"}, "/type"), ({"type": ["integer", 3]}, "/type"), ({"anyOf": [{"type": "integer"}, {"type": "string", "format": "x"}]}, "/anyOf/1/format"),
    ({"type": "object", "properties": {"a": {}}, "required": ["b"]}, "/required"),
    ({"type": "object", "properties": {f"k{i}": {} for i in range(65)}}, "/properties"), ({"unknownKeyword": 1}, "/unknownKeyword"),
]


def test_every_refusal_comes_with_its_path_or_offset(libs):
    pkg, host = libs
    for schema, path in REFUSED:
        with pytest.raises(pkg.hostabi.JsonSchemaError) as e:
            host.json_schema_regex(schema)
        assert (e.value.code, e.value.where) == (-4, path), schema
        with pytest.raises(ref.Refused) as r:
            ref.regex(schema)
        assert r.value.path == path, schema
    for text, offset in [("", 0), ("{", 1), ('{"type": }', 9), ('{"a": 1,}', 8), ('{"a": 01}', 7), ('{"a": "\\x"}', 8), ('{"a": tru}', 9), ("{} x", 3),
                         ('{"a": "\n"}', 7), ('{"a" 1}', 5), ("[1, 2", 5), ('{"a": "\\ud800"}', 13), ("[" * 70 + "]" * 70, 65)]:
        with pytest.raises(pkg.hostabi.JsonSchemaError) as e:
            host.json_schema_regex(text)
        assert (e.value.code, e.value.where) == (-1, offset), text
    for text in ("[]", "3", '"string"', "true"):                          # JSON, but no schema
        with pytest.raises(pkg.hostabi.JsonSchemaError) as e:
            host.json_schema_regex(text)
        assert (e.value.code, e.value.where) == (-4, "/"), text
    for ws, depth in [(2, 2), (-1, 2), (0, 5), (0, -1)]:
        with pytest.raises(pkg.hostabi.JsonSchemaError) as e:
            host.json_schema_regex({}, ws, depth)
        assert (e.value.code, e.value.where) == (-1, None)
    # a schema whose pattern needs more subset states than the dialect allows is add_regex's -2, and leaves the pool as it was
    f = pkg.hostabi.Fsm(host, 4)
    f.set_vocab([b"", b"a", b"{", b"}"])
    wide = {"type": "array", "items": {"type": "array", "items": {"type": "string", "minLength": 200, "maxLength": 255}, "minItems": 200, "maxItems": 255}, "maxItems": 255}
    with pytest.raises(pkg.hostabi.RegexError) as e:
        f.add_json_schema(wide, 0)
    assert e.value.code == -2 and f.n_states == 0
    f.close()


def test_many_optional_properties_stay_quadratic(libs):
    pkg, host = libs
    sizes = []
    for n in (8, 16, 32, 64):
        schema = {"type": "object", "properties": {f"k{i}": {"type": "null"} for i in range(n)}}
        pattern = host.json_schema_regex(schema, 1)
        assert pattern == ref.regex(schema, 1)
        sizes.append(len(pattern))
    assert sizes[3] <= 4.5 * sizes[2] <= 4.5 * 4.5 * sizes[1], sizes      # doubling n at most quadruples it (and some slack for the digits)
    doc = {f"k{i}": None for i in range(64) if i % 3 != 1}
    assert re.fullmatch(pattern, json.dumps(doc), re.ASCII) and re.fullmatch(pattern, "{}", re.ASCII)
    assert not re.fullmatch(pattern, json.dumps({"k1": None, "k0": None}), re.ASCII)
