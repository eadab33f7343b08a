"""Host tokenizer (tinyllama.cpp_amd/host/tokenizer.h) against the reference's tokenizer.h.

The vocabulary file is the reference's data asset, stored byte for byte as tests/golden/tokenizer.bin ($GTEN_TOKENIZER_BIN
overrides it).  Pins:
  * the known answer written in the reference (tinyllama.cpp:101-104),
  * golden ids / pieces produced by the real reference code (tests/golden/make_tokenizer_golden.py),
  * the reference on random text (ASCII, UTF-8, stray continuation bytes) and on every id of the vocabulary: live where
    oracle/_ref is built, elsewhere what it returned for the same texts and ids (tests/golden/tokenizer_live.npz).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from __graft_entry__ import load_package

HERE = os.path.dirname(os.path.abspath(__file__))
VOCAB = os.environ.get("GTEN_TOKENIZER_BIN", os.path.join(HERE, "golden", "tokenizer.bin"))

pytestmark = pytest.mark.skipif(not os.path.exists(VOCAB), reason="tokenizer.bin (the reference's vocabulary file) is not available")


@pytest.fixture(scope="module")
def tok():
    pkg = load_package()
    host = pkg.load_host()
    t = host.tokenizer(VOCAB)
    yield t
    t.close()


def test_known_answer_of_the_reference(tok):
    # tinyllama.cpp:101-104
    assert tok.encode("Who is Karl Marx?") == [1, 32001, 1404, 13, 22110, 338, 8425, 28579, 29973, 32002, 29871, 13, 32001, 20255, 13]


def test_golden_ids_and_pieces(tok):
    pins = json.load(open(os.path.join(HERE, "golden", "tokenizer_pins.json")))
    for e in pins["encode"]:
        assert tok.encode(e["prompt"]) == e["ids"], e["prompt"]
    for prev, token, piece_hex in pins["decode_hex"]:
        assert tok.decode(prev, token).hex() == piece_hex, (prev, token)


def test_chat_template_wraps_the_plain_ids(tok):
    plain = tok.encode("user\nhello there", chat_template=False)
    assert tok.encode("hello there") == [1, 32001] + plain + [32002, 29871, 13, 32001, 20255, 13]
    assert tok.encode("", chat_template=False) == []


def _reference():
    from oracle import orc
    ref = orc.load_ref("avx")
    if ref is None or not hasattr(ref.lib, "ref_tok_create"):
        return None
    L = ref.lib
    L.ref_tok_create.restype = C.c_void_p; L.ref_tok_create.argtypes = [C.c_char_p, C.c_int]
    L.ref_tok_encode.restype = C.c_int; L.ref_tok_encode.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int]
    L.ref_tok_decode.restype = C.c_char_p; L.ref_tok_decode.argtypes = [C.c_void_p, C.c_int, C.c_int]
    return L, L.ref_tok_create(VOCAB.encode(), 32000)


def _split(flat, offs):
    return [flat[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]


def test_against_the_live_reference(tok):
    g = np.load(os.path.join(HERE, "golden", "tokenizer_live.npz"))
    texts = [t.tobytes() for t in _split(g["text_bytes"], g["text_offs"])]
    want_ids = [i.tolist() for i in _split(g["ids"], g["id_offs"])]
    tokens = g["decode_tokens"].tolist()
    want_pieces = [p.tobytes() for p in _split(g["piece_bytes"], g["piece_offs"])]
    assert len(texts) == 300 and len(want_pieces) == 2 * len(tokens)
    r = _reference() if VOCAB.endswith(os.path.join("golden", "tokenizer.bin")) else None
    if r is not None:                             # the live reference: its answers, and the stored ones are still its answers
        L, rt = r
        buf = np.zeros(8192, np.int32)
        for text, want in zip(texts, want_ids):
            cnt = L.ref_tok_encode(rt, text, buf.ctypes.data_as(C.c_void_p), len(buf))
            assert cnt > 0 and buf[:cnt].tolist() == want, text
        assert [L.ref_tok_decode(rt, prev, token) for prev in (0, 1) for token in tokens] == want_pieces
    for text, want in zip(texts, want_ids):
        assert tok.encode(text) == want, text
    got = iter(want_pieces)
    for prev in (0, 1):
        for token in tokens:
            assert tok.decode(prev, token) == next(got), (prev, token)
