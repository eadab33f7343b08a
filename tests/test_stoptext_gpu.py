"""-m gpu: stop strings given as text on the device (include/gten_hip_stoptext.h, include/gten_host_stoptext.h).
Everything here is an equality.  gten_hip_fsm_expand_search against the host expansion byte for byte at the edges of the kernel's tiling,
and against the restatement of tests/stoptext_ref.py where the inputs are ones no builder makes; a mixed pool read back from the device
against the host's view of it; and generation bound to a search range against the UNBOUND generation: the same ids, cut just after the
id that completes the string -- nothing is banned on the way."""
import subprocess

import numpy as np
import pytest

import regex_ref
import stoptext_ref as ref
from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from helpers import F16, Q4, Q8, tiny_config
from test_bias_gpu import SEED, Dec, P
from test_model_gpu import host_cfg
from test_regex_gpu import write_vocab

pytestmark = pytest.mark.gpu

SENTINEL = 0xABCD
CHUNK = 4096                                                             # GTEN_HIP_FSM_EXPAND_CHUNK
LETTERS = b"ab0 1.\n"
# byte states: below, at and above one pass (8: GTEN_HIP_FSM_EXPAND_PASS) and one workgroup's share (64: .._STATES).  A string of
# Sb - 1 bytes makes Sb states; two states need one byte.
STATES = [2, 7, 8, 9, 63, 64, 65]


def stop_of(sb):
    """a string of sb - 1 bytes over LETTERS, the same for every call"""
    g = np.random.default_rng(sb)
    return bytes(g.choice(list(LETTERS), sb - 1).tolist())


def vocab_for(n_vocab):
    """pieces over LETTERS.  255: short pieces (one staged chunk).  256, 257, 513: the first id of a tile is one piece longer than a
    chunk that holds stop_of(7) ACROSS the chunk's edge; 513: the first tile's pieces are 20 bytes each, more than a chunk together.
    Ids 250 .. 252: stop_of(7) with a tail, with a head, and alone (hits in the middle, on the last byte)."""
    s7 = stop_of(7)
    g = np.random.default_rng(n_vocab)
    long_piece = b"x" * (CHUNK - 3) + s7 + b"x" * 9                      # bytes CHUNK - 3 .. CHUNK + 2 of the piece
    if n_vocab == 1:
        return [long_piece], 0
    pieces = regex_ref.synthetic_vocab(n_vocab, 200 + n_vocab, LETTERS)
    long_id = -1
    if n_vocab == 513:
        pieces[8:256] = [bytes(g.choice(list(LETTERS), 20).tolist()) for _ in range(248)]
    if n_vocab >= 256:
        long_id = 0 if n_vocab == 256 else 256
        pieces[long_id] = long_piece
    pieces[250:253] = [s7 + b"zz", b"zz" + s7, s7]
    return pieces, long_id


@pytest.mark.parametrize("n_vocab", [1, 255, 256, 257, 513])
def test_fsm_expand_search_equals_the_host_expansion_byte_for_byte(hip, n_vocab):
    pkg = load_package()
    host = pkg.load_host()
    pieces, long_id = vocab_for(n_vocab)
    vocab = pkg.hostabi.vocab_arrays(pieces)
    f = pkg.hostabi.Fsm(host, n_vocab)
    f.set_vocab(vocab)
    front = np.tile(np.arange(3, dtype=np.uint16)[:, None], (1, n_vocab))
    assert f.add_table(front, np.zeros(3, np.uint8)) == 0                # three host states in front: every range has base > 0
    ranges = []
    for sb in STATES:
        n256, acc = host.stop_text_dfa([stop_of(sb)])
        assert len(acc) == sb
        ranges.append((f.add_stop_text([stop_of(sb)]), n256, acc))
    ranges.append((f.add_stop_text([b"ab", b"b0", b"\n"]), *host.stop_text_dfa([b"ab", b"b0", b"\n"])))
    S = f.n_states + 2                                                   # ... and two rows behind the last range
    want, want_flags = f.tables()
    dn = pkg.hipabi.DeviceBuffer.from_numpy(hip, np.full((S, n_vocab), SENTINEL, np.uint16))
    df = pkg.hipabi.DeviceBuffer.from_numpy(hip, np.full(S + 3, 0xEE, np.uint8))
    pool = (dn, df, S)
    for base, n256, acc in ranges:
        hip.fsm_expand_search(pool, n_vocab, base, vocab, n256, acc)
    got = dn.download(np.uint16, (S, n_vocab))
    got_flags = df.download(np.uint8)[:S + 3]
    assert (got[:3] == SENTINEL).all() and (got[S - 2:] == SENTINEL).all()                    # the rows before and after keep the sentinel
    assert (got_flags[:3] == 0xEE).all() and (got_flags[S - 2:] == 0xEE).all()
    for base, n256, acc in ranges:
        n = len(acc) + 1
        bad = np.argwhere(got[base:base + n] != want[base:base + n])
        assert len(bad) == 0, (len(acc), bad[:5].tolist(), got[base + bad[0][0], bad[0][1]], want[base + bad[0][0], bad[0][1]])
        assert (got_flags[base:base + n] == want_flags[base:base + n]).all(), len(acc)
        assert (got[base:base + n - 1] != ref.DEAD).all()                # nothing is banned
    # the restatement says the same of the 7-state range, and the hits are where they were placed
    base, n256, acc = ranges[1]
    rows, _ = ref.expand(n256, acc, pieces, base)
    assert (got[base:base + 8] == rows).all()
    hit = base + 7
    if long_id >= 0:
        assert got[base][long_id] == hit                                 # across the chunk's edge of a piece longer than a chunk
        assert sum(len(p) for p in pieces[(long_id // 256) * 256:(long_id // 256 + 1) * 256]) > CHUNK
    if n_vocab > 8:
        assert got[base][250] == hit and got[base][251] == hit and got[base][252] == hit                              # middle, last byte, whole piece
        last = pieces.index(stop_of(7)[-1:])
        assert got[base + 5][last] == hit and got[base + 4][last] != hit                                              # the first byte of a 1-byte piece
    if n_vocab == 513:
        assert sum(len(p) for p in pieces[:256]) > CHUNK                 # a tile of ordinary pieces that is staged in several rounds
    # what was built on the device passes the device's check without being copied back
    dn.upload(front)
    dn.upload(np.tile(np.array([0, 1], np.uint16)[:, None], (1, n_vocab)), offset=(S - 2) * n_vocab * 2)
    df.upload(np.zeros(3, np.uint8))
    df.upload(np.zeros(2, np.uint8), offset=S - 2)
    assert hip.fsm_check_dev(pool, n_vocab) == (0, -1)
    f.close()


@pytest.mark.parametrize("n_vocab", [7, 300])
def test_inputs_no_builder_makes_stay_in_bounds_and_follow_the_rule(hip, n_vocab):
    """offsets outside the bytes, running backwards, a told length shorter than the buffer; automata of one state, with entries >= Sb
    and 0xFFFF: "empty piece" and "no edge", as the header says, against the restatement over the pieces the kernel's clamp defines"""
    pkg = load_package()
    g = np.random.default_rng(31 + n_vocab)
    pieces = regex_ref.synthetic_vocab(n_vocab, 77, LETTERS)
    vb, vo = pkg.hostabi.vocab_arrays(pieces)
    total = int(vo[-1])
    odd = vo.copy()
    for i in g.choice(n_vocab + 1, max(n_vocab // 5, 2), replace=False):
        odd[i] = int(g.choice([-5, -1, 0, total + 1, 2 ** 31 - 1, -2 ** 31, int(g.integers(0, total + 1))]))
    automata = [(np.zeros((1, 256), np.uint16), np.zeros(1, np.uint8)),                       # one state that never hits
                (np.zeros((1, 256), np.uint16), np.ones(1, np.uint8)),                        # one state, accepting: every byte hits
                (np.full((1, 256), 0xFFFF, np.uint16), np.zeros(1, np.uint8))]                # one state without an edge
    n256, acc = load_package().load_host().stop_text_dfa([b"ab0", b"1."])
    wild = n256.copy()
    where = g.integers(0, wild.size, 200)
    wild.reshape(-1)[where] = g.choice([len(acc), len(acc) + 1, 0xFFFF, 40000], 200)
    automata.append((wild, acc))
    for offsets, n_bytes in [(vo, total), (odd, total), (odd, total // 2), (vo, 0)]:
        seen = ref.clamp_pieces(vb, offsets, n_bytes)
        if offsets is vo and n_bytes == total:
            assert seen == pieces
        S = sum(len(a) + 1 for _, a in automata) + 2
        dn = pkg.hipabi.DeviceBuffer.from_numpy(hip, np.full((S, n_vocab), SENTINEL, np.uint16))
        df = pkg.hipabi.DeviceBuffer.from_numpy(hip, np.full(S + 3, 0xEE, np.uint8))
        base, placed = 1, []
        for t, a in automata:
            hip.fsm_expand_search((dn, df, S), n_vocab, base, (vb, offsets), t, a, n_bytes=n_bytes)
            placed.append((base, t, a))
            base += len(a) + 1
        got, got_flags = dn.download(np.uint16, (S, n_vocab)), df.download(np.uint8)[:S + 3]
        assert (got[0] == SENTINEL).all() and (got[S - 1] == SENTINEL).all() and got_flags[0] == 0xEE and (got_flags[S - 1:] == 0xEE).all()
        for b, t, a in placed:
            rows, fl = ref.expand(t, a, seen, b)
            assert (got[b:b + len(a) + 1] == rows).all() and (got_flags[b:b + len(a) + 1] == fl).all(), (b, n_bytes)


def test_fsm_expand_search_argument_errors(hip):
    pkg = load_package()
    host = pkg.load_host()
    V = 5
    vocab = pkg.hostabi.vocab_arrays([b"", b"a", b"b", b"ab", b"ba"])
    n256, acc = host.stop_text_dfa([b"ab"])                              # 3 states and the HIT state
    pool = hip.fsm_upload(np.full((4, V), SENTINEL, np.uint16), np.zeros(4, np.uint8))
    for base in (1, -1, 4):
        with pytest.raises(pkg.GtenHipError):
            hip.fsm_expand_search(pool, V, base, vocab, n256, acc)
    assert (pool[0].download(np.uint16, (4, V)) == SENTINEL).all()
    hip.fsm_expand_search(pool, V, 0, vocab, n256, acc)                  # fits exactly
    rows, flags = ref.expand(n256, acc, regex_ref.pieces_of(vocab), 0)
    assert (pool[0].download(np.uint16, (4, V)) == rows).all() and (pool[1].download(np.uint8)[:4] == flags).all()


ALPHABET = bytes(range(0x41, 0x5B)) + b"0123456789 .\n"                   # (few accidental repeats of a 3-byte string in 30 ids)
MODES = [("q4", Q4, Q8), ("f16", F16, F16)]


def setup(host, wd, ad, V=512, max_ctx=64):
    cfg = host_cfg(tiny_config(wd, ad, n_vocab=V, n_heads=4, n_kv_heads=2, max_ctx=max_ctx))
    return cfg, [host.synth_weight(cfg, 4711, i) for i in range(len(cfg.weight_shapes()))]


def straddling_stop(pieces, new_ids, k_from=1, k_only=None):
    """(stop string, k): the bytes from the middle of new piece k to the middle of piece k + 1 -- both of two bytes or more -- such that
    the string occurs nowhere earlier in the new text: its first match ends inside piece k + 1.  None when no k will do."""
    text = b"".join(pieces[i] for i in new_ids)
    ends = np.cumsum([len(pieces[i]) for i in new_ids])
    for k in ([k_only] if k_only is not None else range(k_from, len(new_ids) - 1)):
        a, b = pieces[new_ids[k]], pieces[new_ids[k + 1]]
        if len(a) < 2 or len(b) < 2:
            continue
        stop = a[len(a) // 2:] + b[:(len(b) + 1) // 2]
        _, begin, end = ref.find([stop], text)
        if ends[k] < end <= ends[k + 1] and begin < ends[k]:
            return stop, k
    return None


@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("n_seq", [1, 2, 16])
def test_generation_to_a_text_stop_is_the_unbound_generation_cut_after_the_hit(hip, n_seq, mode):
    pkg = load_package()
    host = pkg.load_host()
    cfg, weights = setup(host, mode[1], mode[2])
    V = cfg.n_vocab
    pieces = regex_ref.synthetic_vocab(V, 9, ALPHABET)
    d = Dec(host, cfg, weights, n_seq)
    prompts = [list(host.synthetic_tokens(P, seed=700 + q, n_vocab=V)) for q in range(n_seq)]
    streams = np.arange(n_seq, dtype=np.uint32) * 7 + 3
    total = P + 30

    def run(st, ks, **kw):
        if d.one:
            ids, ended = d.o.generate_fsm(prompts[0], total, int(st[0]), -1, int(ks[0]), 0.9, SEED, int(streams[0]), **kw)
            return [ids], np.array([ended])
        return d.o.generate_fsm(prompts, total, st, -1, ks, 0.9, SEED, streams, **kw)

    # greedy; top-k with cuts; top-k with penalties
    requests = [(np.zeros(n_seq, np.int32), {}), (np.full(n_seq, 40, np.int32), dict(top_p=0.95, min_p=0.01)),
                (np.full(n_seq, 40, np.int32), dict(rep=1.3, freq=0.1, pres=0.2))]
    hits = 0
    for ks, kw in requests:
        free, free_ended = run(np.full(n_seq, -1, np.int32), ks, **kw)
        assert all(len(x) == total for x in free) and (free_ended == 0).all()
        f = pkg.hostabi.Fsm(host, V)
        f.set_vocab(pieces)
        plans, st = [], []
        for q in range(n_seq):
            new = free[q][P:].tolist()
            found = straddling_stop(pieces, new) if q % 4 != 3 else None
            strings = [found[0], b"\x01never\x02"] if found else [b"\x01never\x02", b"~~~~"]             # q % 4 == 3: strings that never occur
            plans.append((strings, found))
            st.append(f.add_stop_text(strings))
        assert f.n_search == n_seq
        d.o.set_fsm(f)
        ids, ended = run(np.array(st, np.int32), ks, **kw)
        for q, (strings, found) in enumerate(plans):
            new = free[q][P:].tolist()
            text = b"".join(pieces[i] for i in new)
            if found is None:
                assert ids[q].tolist() == free[q].tolist() and ended[q] == 0, q                     # a string that never occurs changes nothing
                assert host.stop_text_find(strings, text) == (-1, len(text), len(text))
                continue
            stop, k = found
            assert ids[q].tolist() == free[q][:P + k + 2].tolist() and ended[q] == 2, (q, k, ids[q].tolist(), free[q].tolist())
            got_text = b"".join(pieces[i] for i in ids[q][P:].tolist())
            cut = host.stop_text_find(strings, got_text)
            assert cut == ref.find(strings, got_text) and cut[0] == 0 and got_text[cut[1]:cut[2]] == stop
            assert cut[2] > len(got_text) - len(pieces[new[k + 1]])                                 # it ends inside the last piece kept
            hits += 1
        f.close()
    assert hits >= 2 * max(n_seq // 2, 1)
    d.o.close()


def test_generate_stop_text_returns_the_text_cut_before_the_string(hip):
    pkg = load_package()
    host = pkg.load_host()
    cfg, weights = setup(host, Q4, Q8)
    pieces = regex_ref.synthetic_vocab(cfg.n_vocab, 9, ALPHABET)
    m = host.model(cfg)
    for i, w in enumerate(weights):
        m.set_weight(i, w)
    prompt = list(host.synthetic_tokens(P, seed=700, n_vocab=cfg.n_vocab))
    free, ended, text = m.generate_stop_text(prompt, P + 30, None, pieces, top_k=40, temp=0.9, seed=SEED, stream=3)
    assert ended == 0 and text == b"".join(pieces[i] for i in free[P:].tolist())
    stop, k = straddling_stop(pieces, free[P:].tolist())
    ids, ended, cut = m.generate_stop_text(prompt, P + 30, [stop], pieces, top_k=40, temp=0.9, seed=SEED, stream=3)
    assert ids.tolist() == free[:P + k + 2].tolist() and ended == 2
    assert cut == text[:text.index(stop)] and not cut.endswith(stop) and stop not in cut
    m.close()


def test_serve_fsm_ends_at_the_hit_around_a_slice_edge_and_in_the_prompt_pass(hip):
    """a queue of prompts through 4 slots in slices of 8 steps.  The first new id comes from the prompt pass and new id j from step j of
    the slot, so hits at new ids 7, 8 and 9 lie one step before, at and one step after the first slice's edge, and 15 / 16 / 17
    around the second; one prompt's string is completed by its first new id, which ends it without a decode step"""
    pkg = load_package()
    host = pkg.load_host()
    cfg, weights = setup(host, Q4, Q8)
    V = cfg.n_vocab
    pieces = regex_ref.synthetic_vocab(V, 9, ALPHABET)
    n = 48
    prompts = [list(host.synthetic_tokens(P + j % 3, seed=800 + j, n_vocab=V)) for j in range(n)]
    bt = host.batch(cfg, 4)
    for i, w in enumerate(weights):
        bt.set_weight(i, w)
    total = P + 2 + 24
    kw = dict(rep=1.2, top_p=0.95, slice_steps=8, max_new_each=[24] * n)
    free, _, free_ended = bt.serve_fsm(prompts, total, -1, 40, 0.9, SEED, -1, **kw)
    assert (free_ended == 0).all()
    # for every wanted position of the completing id one prompt whose unbound text allows it; the others get strings that never occur
    wanted, plans = [7, 8, 9, 15, 16, 17, 0], {}
    for j in range(n):
        new = free[j][len(prompts[j]):].tolist()
        for w in wanted:
            if w in plans.values() or j in plans:
                continue
            if w == 0:
                piece = pieces[new[0]]
                ok = len(piece) >= 2 and ref.find([piece[1:]], b"".join(pieces[i] for i in new))[2] == len(piece)
                found = (piece[1:], -1) if ok else None
            else:
                found = straddling_stop(pieces, new, k_only=w - 1)
            if found:
                plans[j] = w
                prompts[j] = (prompts[j], found[0])
    assert sorted(plans.values()) == sorted(wanted), plans
    f = pkg.hostabi.Fsm(host, V)
    f.set_vocab(pieces)
    st, plain = [], []
    for j in range(n):
        stop = prompts[j][1] if j in plans else b"\x01never\x02"
        plain.append(prompts[j][0] if j in plans else prompts[j])
        st.append(f.add_stop_text([stop]))
    bt.set_fsm(f)
    ids, stats, ended = bt.serve_fsm(plain, total, -1, 40, 0.9, SEED, st, **kw)
    for j in range(n):
        if j in plans:
            keep = len(plain[j]) + plans[j] + 1
            assert ids[j].tolist() == free[j][:keep].tolist() and ended[j] == 2, (j, plans[j])
        else:
            assert ids[j].tolist() == free[j].tolist() and ended[j] == 0, j
    assert stats["admissions"] == n
    # the same through serve_stop_text, which builds the pool itself and cuts the text
    strings = [[prompts[j][1]] if j in plans else None for j in range(n)]
    out = bt.serve_stop_text(plain, strings, -1, pieces, total, 40, 0.9, SEED, **kw)
    for j in range(n):
        assert out[0][j].tolist() == ids[j].tolist() and out[2][j] == ended[j]
        if j in plans:
            assert strings[j][0] not in out[3][j] and out[3][j] + strings[j][0] == b"".join(pieces[i] for i in ids[j][len(plain[j]):].tolist())[:len(out[3][j]) + len(strings[j][0])]
    f.close()
    bt.close()


def test_a_mixed_pool_on_the_device_is_the_hosts_view_row_for_row(hip):
    pkg = load_package()
    host = pkg.load_host()
    cfg, weights = setup(host, Q4, Q8)
    V = cfg.n_vocab
    pieces = regex_ref.synthetic_vocab(V, 9, b'ab01 .\n{}":,truefals')
    f = pkg.hostabi.Fsm(host, V)
    f.set_vocab(pieces)
    s0 = f.add_stop([[5, 6], [7]])
    t0 = f.add_stop_text([b"ab", b"1."])
    r0 = f.add_regex("[ab]+ [01]", 0)
    c0 = f.add_choices([[9, 10], [9, 11, 12], [3]])
    j0 = f.add_json_schema({"type": "object", "properties": {"a": {"type": "boolean"}}, "required": ["a"]}, 0)
    t1 = f.add_stop_text([b"\n"])
    assert s0 == 0 < t0 < r0 < c0 < j0 < t1 and f.n_search == 2 and f.n_regex == 2
    nxt, flags = f.tables()
    bt = host.batch(cfg, 2)
    for i, w in enumerate(weights):
        bt.set_weight(i, w)
    bt.set_fsm(f)
    got, got_flags = hip.decoder_fsm_pool(bt.fsm_decoder(), V)
    assert got.shape == nxt.shape and (got == nxt).all() and (got_flags == flags).all()
    assert hip.fsm_check_dev(hip.fsm_upload(got, got_flags), V) == (0, -1) == hip.fsm_check(nxt, flags, V)
    # the parts interface itself: a search part needs the vocabulary, takes no eos, and is Sb + 1 states
    dec = bt.fsm_decoder()
    n256, acc = host.stop_text_dfa([b"ab"])
    zeros = np.zeros(8, np.uint8)
    hip.decoder_set_vocab_bytes(dec, None)
    assert hip.decoder_set_fsm_parts_ex_rc(dec, 4, zeros[:4], [("search", n256, acc)]) != 0
    hip.decoder_set_vocab_bytes(dec, pkg.hostabi.vocab_arrays(pieces))
    assert hip.decoder_set_fsm_parts_ex_rc(dec, 3, zeros[:3], [("search", n256, acc)]) != 0
    assert hip.decoder_set_fsm_parts_ex_rc(dec, 5, zeros[:5], [("search", n256, acc)]) != 0
    again, _ = hip.decoder_fsm_pool(dec, V)
    assert (again == nxt).all()                                          # a refusal leaves the previous pool
    assert hip.decoder_set_fsm_parts_ex_rc(dec, 4, zeros[:4], [("search", n256, acc)]) == 0
    rows, fl = ref.expand(n256, acc, pieces, 0)
    got, got_flags = hip.decoder_fsm_pool(dec, V)
    assert (got == rows).all() and (got_flags == fl).all()
    f.close()
    bt.close()


def test_the_command_line_prints_what_the_python_calls_return(hip, tmp_path):
    pkg = load_package()
    host = pkg.load_host()
    cfg = host.default_config(4, 3)                       # full-size TinyLlama, q4 weights x q8 activations
    ckpt, vocab = str(tmp_path / "tinyllama.q4.gten"), str(tmp_path / "vocab.bin")
    host.write_gten(cfg, 4242, ckpt)
    write_vocab(vocab)
    n_pred = 40
    tok = host.tokenizer(vocab)
    prompt = tok.encode("hello world")
    cfg2 = host.default_config(4, 3)
    cfg2.max_ctx = n_pred
    m = host.model(cfg2)
    m.load_gten(ckpt)
    pieces = regex_ref.pieces_of(tok.vocab_bytes(cfg.n_vocab))
    free, _, text = m.generate_stop_text(prompt, n_pred, None, tok)
    found = straddling_stop(pieces, free[len(prompt):].tolist())
    assert found is not None, text
    stop = found[0].decode()
    want, ended, cut = m.generate_stop_text(prompt, n_pred, [stop, "\x01never"], tok)
    assert ended == 2 and len(want) == len(prompt) + found[1] + 2
    schema = {"type": "object", "properties": {"name": {"type": "string", "maxLength": 6}, "n": {"type": "integer"}}, "required": ["n"]}
    path = tmp_path / "schema.json"
    import json
    path.write_text(json.dumps(schema))
    jwant, jended = m.generate_json(prompt, n_pred, schema, tok, eos=32002)
    m.close()
    base = [pkg.build.HOST_CLI, "-q4", "-greedy", "--npred", str(n_pred), "--model", ckpt, "--tokenizer", vocab, "-p", "hello world"]
    r = subprocess.run(base + ["--ids", "--stop-text", stop, "--stop-text", "\x01never"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [int(x) for x in r.stdout.split()] == want[len(prompt):].tolist()
    r = subprocess.run(base + ["--stop-text", stop, "--stop-text", "\x01never"], capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stderr.rstrip(b"\n").endswith(cut), r.stderr[-2000:]
    r = subprocess.run(base + ["--ids", "--json-schema", str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [int(x) for x in r.stdout.split()] == jwant[len(prompt):].tolist() and len(jwant) > len(prompt)
