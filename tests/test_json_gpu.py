"""-m gpu: generation held to a JSON schema (include/gten_host_json.h).  A schema is add_regex of its pattern, so
generate_json equals generate_regex of json_schema_regex(schema) id for id; what comes out fullmatches the pattern, passes json.loads
and fits the schema (tests/json_schema_ref.py's validator), greedy and sampled, alone and with two schemas in one serving queue.  The
vocabulary holds every single byte and multi-byte pieces that straddle JSON's punctuation."""
import json
import re

import pytest

import json_schema_ref as ref
from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from test_bias_gpu import SEED, P
from test_nucleus_gpu import model_setup

pytestmark = pytest.mark.gpu

EOS = 0
STRADDLERS = [b'":', b'",', b'"}', b"}]", b'{"', b'":"', b'","', b"],", b"[{", b'":[', b"true", b"false", b"null", b'"name"', b'"n":', b'"tags":["',
              b"ab", b"12", b"-1", b"0.5", b"e+1", b'\\"', b"\\u00e9", "é".encode(), b'a"', b"1,", b"1}", b"1]", b"e}", b'l,"', b"{}", b"[]"]
PERSON = {"type": "object", "properties": {"name": {"type": "string", "maxLength": 5}, "n": {"type": "integer"},
                                           "tags": {"type": "array", "items": {"enum": ["a", "b", "é"]}, "maxItems": 2}, "ok": {"type": ["boolean", "null"]}},
          "required": ["n", "ok"]}
POINTS = {"type": "array", "items": {"type": "object", "properties": {"x": {"type": "integer"}, "y": {"type": "integer"}}, "required": ["x", "y"]},
          "minItems": 1, "maxItems": 2}


def vocabulary(V):
    """id 0 empty (the eos), ids 1 .. 256 the single bytes, then the straddling pieces, the rest empty"""
    pieces = [b""] + [bytes([c]) for c in range(256)] + STRADDLERS
    return pieces + [b""] * (V - len(pieces))


def check(pkg, host, schema, pieces, prompt, ids, ended, total):
    """what a bound sequence may look like: ended by a final state or the eos -> a document that fits; by length -> a prefix of one"""
    pattern = host.json_schema_regex(schema)
    text = b"".join(pieces[i] for i in ids[len(prompt):].tolist())
    n256, acc = pkg.hostabi.byte_dfa(host, pattern)
    s = 0
    for c in text:
        s = int(n256[s][c])
        assert s != 0xFFFF, text
    if ended == 0:
        assert len(ids) == total
        return 0
    doc = text.decode("utf-8")
    assert re.fullmatch(pattern, doc, re.ASCII) is not None, doc
    assert ref.valid(schema, json.loads(doc)), doc
    return 1


def test_generate_json_is_generate_regex_of_the_schemas_pattern_and_fits(hip):
    pkg = load_package()
    host = pkg.load_host()
    cfg, weights = model_setup(host, 512, max_ctx=160)
    pieces = vocabulary(cfg.n_vocab)
    m = host.model(cfg)
    for i, w in enumerate(weights):
        m.set_weight(i, w)
    total, complete = P + 140, 0
    for q, schema in enumerate([PERSON, POINTS, {"enum": ["yes", "no", 7, None]}]):
        prompt = list(host.synthetic_tokens(P, seed=900 + q, n_vocab=cfg.n_vocab))
        for kw in (dict(), dict(top_k=40, temp=0.9, seed=SEED, stream=q), dict(top_k=40, temp=1.2, seed=SEED + 1, stream=q, rep=1.2, top_p=0.9)):
            ids, ended = m.generate_json(prompt, total, schema, pieces, EOS, **kw)
            want, want_ended = m.generate_regex(prompt, total, host.json_schema_regex(schema), pieces, EOS, **kw)
            assert ids.tolist() == want.tolist() and ended == want_ended
            complete += check(pkg, host, schema, pieces, prompt, ids, ended, total)
    assert complete >= 3
    m.close()


def test_serve_json_with_two_schemas_in_one_queue(hip):
    pkg = load_package()
    host = pkg.load_host()
    cfg, weights = model_setup(host, 512, max_ctx=160)
    pieces = vocabulary(cfg.n_vocab)
    bt = host.batch(cfg, 4)
    for i, w in enumerate(weights):
        bt.set_weight(i, w)
    schemas = [PERSON, POINTS, None, POINTS, PERSON, PERSON, POINTS, PERSON, None, POINTS]
    prompts = [list(host.synthetic_tokens(P, seed=950 + j, n_vocab=cfg.n_vocab)) for j in range(len(schemas))]
    total = P + 140
    for kw in (dict(top_k=0), dict(top_k=40, temp=0.9, seed=SEED)):
        ids, stats, ended, starts = bt.serve_json(prompts, schemas, EOS, pieces, total, slice_steps=8, **kw)
        assert len({s for s in starts if s >= 0}) == 2 and starts[2] == starts[8] == -1        # a pool of the two distinct schemas
        patterns = [None if s is None else host.json_schema_regex(s) for s in schemas]
        again = bt.serve_regex(prompts, patterns, EOS, pieces, total, slice_steps=8, **kw)
        complete = 0
        for j, schema in enumerate(schemas):
            assert ids[j].tolist() == again[0][j].tolist() and ended[j] == again[2][j], j
            if schema is not None:
                complete += check(pkg, host, schema, pieces, prompts[j], ids[j], ended[j], total)
        assert complete >= 3
    bt.close()
