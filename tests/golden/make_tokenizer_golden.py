"""Golden vectors of the reference's tokenizer (tokenizer.h) for host/tokenizer.h.

Run in the build container (needs /root/reference and oracle/_ref/libref_avx.so, i.e. __graft_entry__.build()):
    python tests/golden/make_tokenizer_golden.py
writes tests/golden/tokenizer_pins.json: prompts with the ids of Tokenizer::encode (chat template included) and
(prev, token, piece) triples of Tokenizer::decode, and tests/golden/tokenizer_live.npz: the reference's ids of random texts
(ASCII, UTF-8, stray continuation bytes) and its piece of every (prev in {0, 1}, token) pair -- what
tests/test_tokenizer_cpu.py::test_against_the_live_reference holds the host tokenizer to where oracle/_ref is not built.
All produced by the REAL reference code on its own tokenizer.bin (stored byte for byte as tests/golden/tokenizer.bin).
"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import orc  # noqa: E402

VOCAB = os.path.join(ROOT, "tests", "golden", "tokenizer.bin")     # the reference's own file, byte for byte
PROMPTS = [
    "Who is Karl Marx?",                                   # the known answer in tinyllama.cpp:101-104
    "Give three tips for staying healthier.",
    "",
    " ",
    "hello",
    "Hello, world! 12345 -- tabs\tand\nnewlines\r\n",
    "naïve café déjà vu — “quotes” … ¿qué?",
    "日本語のテキストと中文文本",
    "emoji 😀🚀 and rare ᚠᚢᚦ runes",
    "def f(x):\n    return x ** 2  # code\n",
    "a" * 70 + " " + "b" * 3,
    "    leading spaces and trailing   ",
    "MixedCASE_with-symbols+=/\\|<>[]{}()!@#$%^&*~`",
    "The quick brown fox jumps over the lazy dog. " * 3,
]


def main():
    ref = orc.load_ref("avx")
    assert ref is not None and os.path.exists(VOCAB)
    L = ref.lib
    L.ref_tok_create.restype = C.c_void_p; L.ref_tok_create.argtypes = [C.c_char_p, C.c_int]
    L.ref_tok_encode.restype = C.c_int; L.ref_tok_encode.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int]
    L.ref_tok_decode.restype = C.c_char_p; L.ref_tok_decode.argtypes = [C.c_void_p, C.c_int, C.c_int]
    t = L.ref_tok_create(VOCAB.encode(), 32000)
    buf = np.zeros(4096, np.int32)
    enc = []
    for p in PROMPTS:
        n = L.ref_tok_encode(t, p.encode("utf-8"), buf.ctypes.data_as(C.c_void_p), len(buf))
        assert n > 0
        enc.append({"prompt": p, "ids": buf[:n].tolist()})
    dec = []
    rng = np.random.default_rng(7)
    toks = sorted(set([0, 1, 2, 3, 13, 258, 259, 1404, 22110, 29871, 31999, 32000, 32002, 40000]) | set(range(3, 259, 17)) |
                  set(int(x) for x in rng.integers(0, 32000, 80)))
    for tok in toks:
        for prev in (1, 5):
            dec.append([prev, tok, L.ref_tok_decode(t, prev, tok).hex()])
    out = {"vocab_size": 32000, "source": "reference tokenizer.h on /root/reference/tokenizer.bin (oracle/_ref/libref_avx.so)",
           "encode": enc, "decode_hex": dec}
    path = os.path.join(ROOT, "tests", "golden", "tokenizer_pins.json")
    with open(path, "w") as f:
        json.dump(out, f, ensure_ascii=True, indent=0)
    print("wrote", path, len(enc), "prompts,", len(dec), "decodes")
    live(L, t)


def random_texts():
    """the texts of test_against_the_live_reference: 300 random strings, every tenth with stray / truncated UTF-8 bytes"""
    rng = np.random.default_rng(11)
    alphabet = list("abcdefghijklmnopqrstuvwxyz ABCDEFG 0123456789 .,;:!?'\"()-_\n\t") + ["é", "ß", "ø", "日", "本", "語", "😀", "→", "ᚠ", "  ", "the ", "ing "]
    texts = []
    for trial in range(300):
        n = int(rng.integers(0, 120))
        text = "".join(alphabet[int(i)] for i in rng.integers(0, len(alphabet), n)).encode("utf-8")
        if trial % 10 == 9:                       # stray continuation / truncated lead bytes
            raw = bytearray(text)
            for _ in range(3):
                raw.insert(int(rng.integers(0, len(raw) + 1)), int(rng.choice([0x80, 0xBF, 0xC3, 0xE2, 0xF0])))
            text = bytes(b for b in raw if b != 0)
        texts.append(text)
    return texts


DECODE_TOKENS = list(range(0, 32000)) + [32000, 32001, 32002, 40000]


def packed(chunks, dtype):
    """a list of arrays / byte strings -> (concatenation, offsets)"""
    offs = np.cumsum([0] + [len(c) for c in chunks]).astype(np.int64)
    flat = np.concatenate([np.frombuffer(c, np.uint8) if isinstance(c, bytes) else np.asarray(c) for c in chunks] or [np.zeros(0)])
    return flat.astype(dtype), offs


def unpacked(flat, offs):
    return [flat[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]


def live(L, t):
    texts = random_texts()
    buf = np.zeros(8192, np.int32)
    ids = []
    for text in texts:
        n = L.ref_tok_encode(t, text, buf.ctypes.data_as(C.c_void_p), len(buf))
        assert n > 0
        ids.append(buf[:n].copy())
    pieces = [L.ref_tok_decode(t, prev, tok) for prev in (0, 1) for tok in DECODE_TOKENS]
    text_bytes, text_offs = packed(texts, np.uint8)
    id_vals, id_offs = packed(ids, np.int32)
    piece_bytes, piece_offs = packed(pieces, np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "tokenizer_live.npz")
    np.savez_compressed(path, text_bytes=text_bytes, text_offs=text_offs, ids=id_vals, id_offs=id_offs,
                        decode_tokens=np.array(DECODE_TOKENS, np.int32), piece_bytes=piece_bytes, piece_offs=piece_offs)
    print("wrote", path, len(texts), "texts,", len(pieces), "pieces")


if __name__ == "__main__":
    main()
