"""-m gpu: byte automata expanded over the vocabulary on the device (include/gten_hip_regex.h, include/gten_host_regex.h, DESIGN.md
3.18).  Everything here is an equality: gten_hip_fsm_expand against the host expansion byte for byte at the shapes where a tiling can go
wrong; gten_hip_fsm_check_dev against gten_hip_fsm_check; generation bound to a range that was expanded on the device against the same
automaton materialised on the host and uploaded as a table; a mixed pool read back from the device against the host's view of it;
and the command line against the Python path.  The end-to-end test holds what was generated to Python's re."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import fsm_ref
import regex_ref as ref
from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from test_bias_gpu import SEED, Dec, P
from test_nucleus_gpu import model_setup

pytestmark = pytest.mark.gpu

SENTINEL = 0xABCD
# Sb 1 (with and without an edge), 2, 3 (a loop that survives a piece of any length), 71 (above the 64 states one workgroup covers:
# GTEN_HIP_FSM_EXPAND_STATES) and 257
SHAPES = [("a{0}", 1), ("a*", 1), ("a+", 2), ("(aaa)*", 3), ("[ab]{70}", 71), ("a{255}b", 257), ("([ab01]+[ .\n])*", 2)]


def vocab_for(n_vocab, hipabi):
    """empty pieces, 1-byte pieces, a piece one byte longer than the kernel's staging chunk and one of 200 bytes; the total number of
    bytes -- the largest offset -- is not a multiple of 4"""
    chunk = hipabi.GtenHip.FSM_EXPAND_CHUNK
    pieces = ref.synthetic_vocab(n_vocab, 100 + n_vocab, long_piece=chunk + 1, extra=[b"a" * 200, b"ab"] if n_vocab > 8 else [])
    if n_vocab == 1:
        pieces = [b"a" * (chunk + 1)]
    while sum(len(p) for p in pieces) % 4 == 0:
        pieces[-1] = pieces[-1] + b"a"
    return pieces


@pytest.mark.parametrize("n_vocab", [1, 255, 256, 257, 4099, 32003])
def test_fsm_expand_equals_the_host_expansion_byte_for_byte(hip, n_vocab):
    pkg = load_package()
    host = pkg.load_host()
    pieces = vocab_for(n_vocab, pkg.hipabi)
    vocab = pkg.hostabi.vocab_arrays(pieces)
    assert vocab[1][-1] % 4 != 0 and min(len(p) for p in pieces) == 0 or n_vocab == 1
    f = pkg.hostabi.Fsm(host, n_vocab)
    f.set_vocab(vocab)
    front = np.tile(np.arange(3, dtype=np.uint16)[:, None], (1, n_vocab))
    assert f.add_table(front, np.zeros(3, np.uint8)) == 0                # three host states in front: every range has base > 0
    ranges = []
    for p, sb in SHAPES:
        n256, acc = pkg.hostabi.byte_dfa(host, p)
        assert len(acc) == sb, (p, len(acc))
        for eos in sorted({-1, 0, n_vocab - 1}):
            ranges.append((f.add_regex(p, eos), n256, acc, eos, p))
    S = f.n_states + 2                                                   # ... and two rows behind the last range
    want, want_flags = f.tables()
    dn = pkg.hipabi.DeviceBuffer.from_numpy(hip, np.full((S, n_vocab), SENTINEL, np.uint16))
    df = pkg.hipabi.DeviceBuffer.from_numpy(hip, np.full(S + 3, 0xEE, np.uint8))
    pool = (dn, df, S)
    for base, n256, acc, eos, p in ranges:
        hip.fsm_expand(pool, n_vocab, base, vocab, n256, acc, eos)
    got = dn.download(np.uint16, (S, n_vocab))
    got_flags = df.download(np.uint8)[:S + 3]
    assert (got[:3] == SENTINEL).all() and (got[S - 2:] == SENTINEL).all()                    # the rows before and after keep the sentinel
    assert (got_flags[:3] == 0xEE).all() and (got_flags[S - 2:] == 0xEE).all()
    for base, n256, acc, eos, p in ranges:
        n = len(acc) + (eos >= 0)
        bad = np.argwhere(got[base:base + n] != want[base:base + n])
        assert len(bad) == 0, (p, eos, bad[:5].tolist(), got[base + bad[0][0], bad[0][1]], want[base + bad[0][0], bad[0][1]])
        assert (got_flags[base:base + n] == want_flags[base:base + n]).all(), (p, eos)
    # the long pieces were walked to their end, not cut at a chunk's edge: a* and (aaa)* survive them, a+ too
    long_id = 0 if n_vocab == 1 else n_vocab // 2
    if n_vocab > 2:
        assert len(pieces[long_id]) >= hip.FSM_EXPAND_CHUNK + 1
        for base, n256, acc, eos, p in ranges:
            if p in ("a*", "a+", "(aaa)*") and eos != long_id:
                assert got[base][long_id] == base + ref_state(n256, pieces[long_id]), p
    # what was built on the device passes the device's check without being copied back
    head = np.tile(np.arange(3, dtype=np.uint16)[:, None], (1, n_vocab))
    dn.upload(head)
    dn.upload(np.tile(np.array([0, 1], np.uint16)[:, None], (1, n_vocab)), offset=(S - 2) * n_vocab * 2)
    df.upload(np.zeros(3, np.uint8))
    df.upload(np.zeros(2, np.uint8), offset=S - 2)
    full = np.concatenate([want, np.tile(np.array([0, 1], np.uint16)[:, None], (1, n_vocab))])
    full_flags = np.concatenate([want_flags, np.zeros(2, np.uint8)])
    assert hip.fsm_check_dev(pool, n_vocab) == hip.fsm_check(full, full_flags, n_vocab)
    f.close()


def ref_state(n256, data):
    s = 0
    for c in data:
        s = int(n256[s][c])
        if s == ref.NONE:
            break
    return s


def test_fsm_expand_argument_errors(hip):
    pkg = load_package()
    host = pkg.load_host()
    V = 5
    vocab = pkg.hostabi.vocab_arrays([b"", b"a", b"b", b"ab", b"ba"])
    n256, acc = pkg.hostabi.byte_dfa(host, "a+b")
    pool = hip.fsm_upload(np.full((4, V), SENTINEL, np.uint16), np.zeros(4, np.uint8))
    for base, eos in [(2, -1), (1, 0), (-1, -1), (0, 5), (0, -2)]:       # the range leaves the pool; an eos outside the vocabulary
        with pytest.raises(pkg.GtenHipError):
            hip.fsm_expand(pool, V, base, vocab, n256, acc, eos)
    assert (pool[0].download(np.uint16, (4, V)) == SENTINEL).all()
    hip.fsm_expand(pool, V, 0, vocab, n256, acc, 0)                      # 3 states and END fit exactly
    assert (pool[0].download(np.uint16, (4, V)) != SENTINEL).all()


def test_the_device_check_says_what_the_host_check_says(hip):
    pkg = load_package()
    V, S = 4099, 70
    nxt, flags = fsm_ref.random_pool(np.random.default_rng(3), S, V, 0.25, 2)
    cases = {"good": (nxt, flags)}
    bad = nxt.copy()
    bad[S - 1, V - 1] = S                                                # one bad entry in the last state's last column
    cases["bad entry"] = (bad, flags)
    stuck = nxt.copy()
    stuck[41] = fsm_ref.DEAD                                             # one stuck state
    cases["stuck"] = (stuck, flags)
    both = stuck.copy()
    both[50, 7] = 65000                                                  # the first offender in state order is what both report
    both[12, 0] = S + 1
    cases["first of several"] = (both, flags)
    final_dead = nxt.copy()
    final_dead[S - 1] = fsm_ref.DEAD                                     # a final state may allow nothing
    cases["final and dead"] = (final_dead, flags)
    want = {"good": (0, -1), "bad entry": (3, S - 1), "stuck": (4, 41), "first of several": (3, 12), "final and dead": (0, -1)}
    for name, (n, fl) in cases.items():
        host_says = hip.fsm_check(n, fl, V)
        assert host_says == want[name], name
        assert hip.fsm_check_dev(hip.fsm_upload(n, fl), V) == host_says, name
    pool = hip.fsm_upload(nxt, flags)
    assert hip.fsm_check_dev(pool, V, n_states=0)[0] == 1 and hip.fsm_check_dev(pool, V, n_states=65536)[0] == 1      # BAD_STATES, as on the host
    assert hip.fsm_check_dev(pool, 1 << 20, n_states=60000)[0] == 2                                                    # TOO_LARGE


ALPHABET = b"ab01 .\n"
# over the synthetic vocabulary: a few words, a number and a full stop (ends in a state with no way on: FINAL); words for as long as
# the model likes (every accepting state goes on: it ends by eos, through END); one of three answers and an optional tail
GEN_PATTERNS = [r"([ab]+ ){1,3}[01]{2}\.", r"[ab01]+( [ab01]+)*", r"(ab|ba|0+1)(\.\n)?"]
EOS = 0                                                                  # (id 0 spells nothing in the synthetic vocabulary)


def pools_for(pkg, host, V, pieces):
    """the same automata twice: `a` keeps the patterns as byte automata (set_fsm sends them through gten_hip_decoder_set_fsm_parts and
    the device's expansion), `b` holds a's host view as a table the caller brought (add_table + the table route)"""
    a = pkg.hostabi.Fsm(host, V)
    a.set_vocab(pieces)
    starts = [a.add_regex(p, EOS) for p in GEN_PATTERNS]
    nxt, flags = a.tables()
    b = pkg.hostabi.Fsm(host, V)
    assert b.add_table(nxt, flags) == 0 and a.n_regex == 3 and b.n_regex == 0
    return a, b, starts, nxt, flags


@pytest.mark.parametrize("n_seq", [1, 16])
def test_generation_in_an_expanded_range_equals_the_table_route(hip, n_seq):
    pkg = load_package()
    host = pkg.load_host()
    cfg, weights = model_setup(host, 512, max_ctx=64)
    V = cfg.n_vocab
    pieces = ref.synthetic_vocab(V, 9, ALPHABET)
    a, b, starts, nxt, flags = pools_for(pkg, host, V, pieces)
    d = Dec(host, cfg, weights, n_seq)
    prompts = [list(host.synthetic_tokens(P, seed=700 + q, n_vocab=V)) for q in range(n_seq)]
    st = np.array([starts[q % 3] if q % 5 != 4 else -1 for q in range(n_seq)], np.int32)
    streams = np.arange(n_seq, dtype=np.uint32) * 7 + 3
    total = P + 30

    def run(pool, ks, **kw):
        d.o.set_fsm(pool)
        if d.one:
            out = d.o.generate_fsm(prompts[0], total, int(st[0]), -1, int(ks[0]), 0.9, SEED, int(streams[0]), n_top=3, **kw)
            ids, ended, recs = [out[0]], np.array([out[1]]), [out[2:]]
            rows = [d.o.fsm_states(P, len(out[0]) - P + 1)]
        else:
            ids, ended = d.o.generate_fsm(prompts, total, st, -1, ks, 0.9, SEED, streams, **kw)
            recs = [()]                                                  # (the batch's records are serve_fsm's: the test below)
            rows = [d.o.fsm_states(q, P, len(ids[q]) - P + 1) for q in range(n_seq)]
        return ids, ended, recs, rows

    finals = 0
    for ks, kw in [(np.zeros(n_seq, np.int32), {}), (np.full(n_seq, 40, np.int32), dict(top_p=0.9, min_p=0.02, rep=1.3, freq=0.1, pres=0.2))]:
        ia, ea, ra, sa = run(a, ks, **kw)
        ib, eb, rb, sb = run(b, ks, **kw)
        assert ea.tolist() == eb.tolist()
        for q in range(n_seq):
            assert ia[q].tolist() == ib[q].tolist() and sa[q].tolist() == sb[q].tolist(), q
            if st[q] >= 0:                                               # ... and it is the automaton's walk, never a banned id
                walk = fsm_ref.walk(nxt, flags, int(st[q]), ia[q][P:].tolist())
                assert fsm_ref.DEAD not in walk and sa[q][1:].tolist() == walk, q
                finals += ea[q] == 2
        for x, y in zip(ra[0], rb[0]):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()    # the log-prob records, bit for bit
    assert finals >= 1
    # the pool the decoder holds after the device's expansion is the host's view of it, row for row
    if not d.one:
        d.o.set_fsm(a)
        got, got_flags = hip.decoder_fsm_pool(d.o.fsm_decoder(), V)
        assert (got == nxt).all() and (got_flags == flags).all()
    a.close()
    b.close()
    d.o.close()


def test_serve_fsm_through_restarted_slots_equals_the_table_route(hip):
    """a queue of 21 prompts through 16 slots in slices of 8 steps: slots restart with other patterns' start states"""
    pkg = load_package()
    host = pkg.load_host()
    cfg, weights = model_setup(host, 512, max_ctx=64)
    V = cfg.n_vocab
    pieces = ref.synthetic_vocab(V, 9, ALPHABET)
    a, b, starts, nxt, flags = pools_for(pkg, host, V, pieces)
    n = 21
    prompts = [list(host.synthetic_tokens(P + j % 3, seed=800 + j, n_vocab=V)) for j in range(n)]
    st = [starts[j % 3] if j % 4 != 3 else -1 for j in range(n)]
    bt = host.batch(cfg, 16)
    for i, w in enumerate(weights):
        bt.set_weight(i, w)
    total = P + 2 + 24
    out = {}
    for name, pool in (("parts", a), ("table", b)):
        bt.set_fsm(pool)
        out[name] = bt.serve_fsm(prompts, total, -1, 40, 0.9, SEED, st, rep=1.2, top_p=0.95, slice_steps=8, max_new_each=[24] * n, n_top=2)
    (ia, sta, ea, *ra), (ib, stb, eb, *rb) = out["parts"], out["table"]
    assert sta["admissions"] == n and ea.tolist() == eb.tolist() and (ea == 2).sum() >= 2
    for j in range(n):
        assert ia[j].tolist() == ib[j].tolist(), j
        if st[j] >= 0:
            assert fsm_ref.DEAD not in fsm_ref.walk(nxt, flags, st[j], ia[j][len(prompts[j]):].tolist()), j
    for x, y in zip(ra, rb):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    a.close()
    b.close()
    bt.close()


def test_serve_regex_end_to_end(hip):
    pkg = load_package()
    host = pkg.load_host()
    cfg, weights = model_setup(host, 512, max_ctx=64)
    V = cfg.n_vocab
    pieces = ref.synthetic_vocab(V, 9, ALPHABET)
    bt = host.batch(cfg, 4)
    for i, w in enumerate(weights):
        bt.set_weight(i, w)
    patterns = [GEN_PATTERNS[0], GEN_PATTERNS[1], None, GEN_PATTERNS[2], GEN_PATTERNS[0], GEN_PATTERNS[2], GEN_PATTERNS[1], GEN_PATTERNS[0]]
    prompts = [list(host.synthetic_tokens(P, seed=900 + j, n_vocab=V)) for j in range(8)]
    total = P + 40
    ids, stats, ended, starts = bt.serve_regex(prompts, patterns, EOS, pieces, total, 40, 0.9, SEED, slice_steps=8)
    assert len(set(s for s in starts if s >= 0)) == 3 and starts[2] == -1 and starts[0] == starts[4] == starts[7]     # a pool of the distinct patterns
    assert bt.fsm_info()[0] == sum(len(pkg.hostabi.byte_dfa(host, p)[1]) + 1 for p in GEN_PATTERNS)
    complete = 0
    for j, p in enumerate(patterns):
        new = ids[j][P:].tolist()
        if p is None:
            continue
        n256, acc = pkg.hostabi.byte_dfa(host, p)
        text = b"".join(pieces[i] for i in new)
        s = 0
        for c in text:                                                   # the id prefix walks the byte automaton without dying
            s = int(n256[s][c])
            assert s != ref.NONE, (j, text)
        assert all(len(pieces[i]) > 0 or i == EOS for i in new), j       # never an empty piece, but the eos that ends it
        if ended[j] in (1, 2):                                           # ended by the eos in a state that may stop (1: the eos is not kept),
            complete += 1                                                # or by entering a final state (2): the text is one re accepts
            assert re.fullmatch(p, text.decode(), re.ASCII) is not None, (j, p, text, int(ended[j]))
        else:
            assert len(ids[j]) == total, j
    assert complete >= 3
    plain, _, pe = bt.serve_fsm(prompts, total, EOS, 40, 0.9, SEED, -1, slice_steps=8)
    assert ids[2].tolist() == plain[2].tolist() and ended[2] == pe[2]    # the unbound item is plain serve_fsm's
    assert any(ids[j].tolist() != plain[j].tolist() for j in range(8) if patterns[j] is not None)
    bt.close()


def test_a_mixed_pool_on_the_device_is_the_hosts_view_row_for_row(hip):
    pkg = load_package()
    host = pkg.load_host()
    cfg, weights = model_setup(host, 512, max_ctx=64)
    V = cfg.n_vocab
    pieces = ref.synthetic_vocab(V, 9, ALPHABET)
    f = pkg.hostabi.Fsm(host, V)
    f.set_vocab(pieces)
    s0 = f.add_stop([[5, 6], [7]])
    r0 = f.add_regex(GEN_PATTERNS[0], EOS)
    c0 = f.add_choices([[9, 10], [9, 11, 12], [3]])
    r1 = f.add_regex(GEN_PATTERNS[1], -1)
    s1 = f.add_stop([[400, 401, 402]])
    assert [s0, r0] == [0, 4] and c0 < r1 < s1 and f.n_regex == 2
    nxt, flags = f.tables()
    bt = host.batch(cfg, 2)
    for i, w in enumerate(weights):
        bt.set_weight(i, w)
    bt.set_fsm(f)
    got, got_flags = hip.decoder_fsm_pool(bt.fsm_decoder(), V)
    assert got.shape == nxt.shape and (got == nxt).all() and (got_flags == flags).all()
    # a pool the device's check refuses leaves the previous one: no piece spells "c", so the state behind "a" is stuck
    g = pkg.hostabi.Fsm(host, V)
    g.set_vocab(pieces)
    g.add_stop([[1]])
    bad = g.add_regex("ac")
    assert bt.set_fsm_rc(g) != 0 and f"state {bad + 1} is not final and allows no id" in host.hip._err().decode()
    again, _ = hip.decoder_fsm_pool(bt.fsm_decoder(), V)
    assert bt.fsm_info()[0] == f.n_states and (again == nxt).all()
    # ... and so does a pool set while a sequence is bound
    bt.set_seq_fsm(0, r0, 5)
    assert bt.set_fsm_rc(f) != 0
    bt.set_seq_fsm(0, -1)
    bt.set_fsm(f)
    # a regex part needs the vocabulary on the decoder; parts must tile the pool
    dec = bt.fsm_decoder()
    n256, acc = pkg.hostabi.byte_dfa(host, "a+")
    hip.decoder_set_vocab_bytes(dec, None)
    assert hip.decoder_set_fsm_parts_rc(dec, 2, np.zeros(2, np.uint8), [("regex", n256, acc, -1)]) != 0
    hip.decoder_set_vocab_bytes(dec, pkg.hostabi.vocab_arrays(pieces))
    assert hip.decoder_set_fsm_parts_rc(dec, 3, np.zeros(3, np.uint8), [("regex", n256, acc, -1)]) != 0
    assert hip.decoder_set_fsm_parts_rc(dec, 2, np.zeros(2, np.uint8), [("regex", n256, acc, -1)]) == 0
    assert hip.decoder_fsm_pool(dec, V)[0].shape == (2, V)
    f.close()
    g.close()
    bt.close()


def write_vocab(path):
    """tests/test_cli_gpu.py's synthetic vocabulary file: <unk>, <s>, </s>, the 256 byte pieces, printable characters, a few merges"""
    pieces = ["<unk>", "<s>", "</s>"] + [f"<0x{b:02X}>" for b in range(256)]
    singles = [chr(c) for c in range(32, 127)] + ["\n", "\t"]
    merges = ["he", "ll", "lo", "hell", "hello", " w", "or", "ld", " wor", " world", "us", "er", "user", "user\n", " h", " hello"]
    pieces += singles + merges
    while len(pieces) < 32000:
        pieces.append(f"@@{len(pieces)}@@")
    scores = [0.0] * len(pieces)
    for i, m in enumerate(merges):
        scores[pieces.index(m)] = -float(i + 1)
    with open(path, "wb") as f:
        f.write(struct.pack("<i", max(len(p.encode()) for p in pieces)))
        for p, s in zip(pieces, scores):
            b = p.encode()
            f.write(struct.pack("<fi", s, len(b)))
            f.write(b)


def test_the_command_line_prints_the_ids_of_the_python_path(hip, tmp_path):
    pkg = load_package()
    host = pkg.load_host()
    cfg = host.default_config(4, 3)                       # full-size TinyLlama, q4 weights x q8 activations
    ckpt, vocab = str(tmp_path / "tinyllama.q4.gten"), str(tmp_path / "vocab.bin")
    host.write_gten(cfg, 4242, ckpt)
    write_vocab(vocab)
    n_pred, pattern = 40, r"(hello|[a-z]{2,6})( [a-z]+){1,2}\."
    r = subprocess.run([pkg.build.HOST_CLI, "-q4", "-greedy", "--ids", "--npred", str(n_pred), "--model", ckpt, "--tokenizer", vocab, "--regex", pattern,
                        "-p", "hello world"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [int(x) for x in r.stdout.split()]
    tok = host.tokenizer(vocab)
    prompt = tok.encode("hello world")
    cfg2 = host.default_config(4, 3)
    cfg2.max_ctx = n_pred
    m = host.model(cfg2)
    m.load_gten(ckpt)
    want, ended = m.generate_regex(prompt, n_pred, pattern, tok, eos=32002)
    m.close()
    assert got == want[len(prompt):].tolist() and len(got) > 0
    pieces = ref.pieces_of(tok.vocab_bytes(cfg.n_vocab))
    text = b"".join(pieces[i] for i in got).decode()
    n256, acc = pkg.hostabi.byte_dfa(host, pattern)
    assert ref_state(n256, text.encode()) != ref.NONE and (ended == 0 or re.fullmatch(pattern, text, re.ASCII) is not None)
