"""-m gpu: the multi-sequence decoder at the widths where its kernels switch form.

The wide step (16+ sequences, csrc/gten_decode.hip: enqueue_step_wide) does not run one kernel per projection: a K split
(`ks_of`), the f16 K-plane kernels (`wxp_shape`), the streamed gate | up and the lanes of 128 rows are each chosen from the
model's widths.  At the tiny model's 256 none of them is on, at TinyLlama's 2048 all of them are; this file runs the shapes
in between, each switch on in one shape and off in a neighbour (the comment on each row of SHAPES names the branches it takes):

  a. against the oracle (marked oracle_parity: collected first): batch sizes 1, 8, 64 and a lane batch, the sequences on
     both sides of the lane seams, the bands of test_model_gpu.check_logits; one longer case per dtype across the
     256-position attention chunk boundary;
  b. bit identity only where the library promises it: 8 sequences == the single-sequence decoder; set_ffn_streamed(1) ==
     set_ffn_streamed(0); lanes == separate 64-sequence decoders; graph replay == eager launches; f16 wide decoders whose
     lanes split every projection alike (include/gten_hip.h, gten_hip_set_wx_planes).  q4 / q8 wide decoders of different
     sizes are NOT compared bit for bit: nothing promises it (the oracle band holds them);
  c. evidence that the branch named in SHAPES ran: the launch count of the gate | up family in one eager step.

Sequence q always decodes the token stream of seed SEED + q with the same weights, whatever the batch, so one device run
and one oracle run per (shape, dtype, sequence) serve every comparison: both are cached for the module."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from helpers import MODES, tiny_config
from test_model_gpu import check_logits, host_cfg

pytestmark = pytest.mark.gpu

# name: (n_embd, n_ffn, n_heads, n_kv_heads, n_vocab, lane batch).  n_layers 2, d_head 64 everywhere.  ks_of(d): two K planes
# iff d % 512 == 0; planes: wxp_shape (o, down: d_in / 256, q|k|v: d_in / 128 in {1, 2, 3, 4, 6, 8, 16, 22}; q|k|v also 1, 2, 4
# or 8 heads per group -- which is also what keeps head-major shadows).  "gate|up streamed": the one-launch form at 49-64 / 128
# rows; q8 and f16 take it at n_embd 2048 only, q4 always fuses gate | up into one launch.
SHAPES = {
    # K split on E (512) and F (1536); f16 planes for o (NBK 2), down (6) and q|k|v (4; 4 heads per group); gate|up: the slab
    # pair for q8 / f16 (E != 2048); 192 = three lanes of 64 for every dtype
    "A": (512, 1536, 8, 2, 512, 192),
    # K split on E, none on F (2816 / 32 = 88 steps); o planes (4) and q|k|v planes (8; 8 heads per group), down planes OFF
    # (2816 / 256 = 11); a ragged lm_head tile (16403 columns), not streamed (d_in != 2048); 128 = one lane of 128 rows for
    # q4 / q8, two of 64 for f16
    "B": (1024, 2816, 16, 2, 16403, 128),
    # 3 heads per group: per-head attention, no shadows, q|k|v planes OFF -- q|k|v split in K up to 32 rows only; o (6) and
    # down (16) planes on; K split on E and F
    "C": (1536, 4096, 24, 8, 512, 192),
    # everything off: no K split on E (1792 / 32 = 56), no planes (7, 24, 14), no streamed gate|up, 7 heads per group
    # (per-head attention); n_ffn at the decoder's maximum (split in K: 6144 / 32 = 192) -- past a q8 down projection's weight
    # slab (5632): q8 runs here with 1 and 8 sequences only, and a wider q8 decoder is refused (WIDE)
    "D": (1792, 6144, 28, 4, 512, 192),
    # full width, 1 head per group: q|k|v planes (16), o planes (8), down planes OFF (1280 / 256 = 5); gate|up streamed for
    # q8 and f16 (F / 32 = 40 workgroups); lanes of 128 rows for every dtype (f16 only at this width)
    "E": (2048, 1280, 32, 32, 512, 128),
}
LAYERS, MAX_CTX, SEED, WSEED = 2, 272, 6100, 97
SHORT, LONG = 32, 262
CHECKS = (1, 2, 17, 32)
LONG_CHECKS = (1, 2, 100, 255, 256, 257, 262)
STREAM = LONG + 2                       # every stream has this length: the short runs decode a prefix of the long ones
SEAMS = (0, 7, 15, 63, 64, 127, 128, 191)     # sequences whose logits are kept in full (the others: a digest)
MODE = {m[0]: m for m in MODES()}


def ocfg_of(shape, mode):
    E, F, H, KV, V, _ = SHAPES[shape]
    _, wd, ad = MODE[mode]
    return tiny_config(wd, ad, n_embd=E, n_ffn=F, n_heads=H, n_kv_heads=KV, n_vocab=V, max_ctx=MAX_CTX, n_layers=LAYERS)


# ---------------------------------------------------------------- the predicates of enqueue_step_wide / decoder_build, restated

def ks_of(d):
    return 2 if (d // 32) % 16 == 0 else 1


def lane_rows(shape, mode, S):
    """rows per lane of an S-sequence decoder (decoder_build: 128 for q4 / q8 at any width, for f16 only at n_embd 2048)"""
    if S <= 64:
        return S
    return 128 if S % 128 == 0 and (mode != "f16" or SHAPES[shape][0] == 2048) else 64


def f16_qkv_planes(shape):
    E, _, H, KV, _, _ = SHAPES[shape]
    return (E // 128) in (1, 2, 3, 4, 6, 8, 16, 22) and H // KV in (1, 2, 4, 8)


def f16_split(shape, S):
    """(K planes of gate | up, of q | k | v -- 0: the four-plane kernel) of every lane of an f16 S-sequence decoder"""
    E = SHAPES[shape][0]
    r = lane_rows(shape, "f16", S)
    ks_gu = 1 if (r + 15) // 16 == 2 else ks_of(E)
    ks_qkv = 0 if f16_qkv_planes(shape) else (ks_of(E) if r <= 32 else 1)
    return ks_gu, ks_qkv


def gate_up_launches(shape, mode, S):
    """launches of the gate | up family in one step: per layer and lane ONE for the streamed / fused forms, TWO for the slab
    pair (the W.x launch + the silu . mul launch)"""
    E, F = SHAPES[shape][:2]
    r = lane_rows(shape, mode, S)
    lanes = S // r
    if mode == "q4":
        per = 1
    else:
        rt = (r + 15) // 16
        ks_gu = 1 if rt == 2 else ks_of(E)
        per = 1 if (E == 2048 and (rt == 4 or r == 128) and ks_gu == 2 and F % 32 == 0) else 2
    return LAYERS * lanes * per


def lane_batch(shape):
    return SHAPES[shape][5]


# ---------------------------------------------------------------- cached runs

_W, _STREAMS, _DEV, _ORC = {}, {}, {}, {}


def _weights(shape, mode):
    if (shape, mode) not in _W:
        host = load_package().load_host()
        cfg = host_cfg(ocfg_of(shape, mode))
        _W[(shape, mode)] = [host.synth_weight(cfg, WSEED, i) for i in range(len(cfg.weight_shapes()))]
    return _W[(shape, mode)]


def _stream(shape, q):
    key = (SHAPES[shape][4], q)
    if key not in _STREAMS:
        _STREAMS[key] = load_package().load_host().synthetic_tokens(STREAM, seed=SEED + q, n_vocab=SHAPES[shape][4])
    return _STREAMS[key]


def _digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def device_run(hip, shape, mode, S, first=0, n_last=SHORT, checks=CHECKS, graph=True, streamed=True):
    """an S-sequence decoder holding sequences first .. first + S - 1 (S == 1: the single-sequence decoder): at every check
    step {sequence: (device id, logits digest)} and the full logits of the SEAMS sequences"""
    key = (shape, mode, S, first, n_last, graph, streamed)
    if key in _DEV:
        return _DEV[key]
    host = load_package().load_host()
    cfg = host_cfg(ocfg_of(shape, mode))
    qs = range(first, first + S)
    out = {n: ({}, {}) for n in checks}
    hip.set_ffn_streamed(streamed)
    try:
        if S == 1:
            m = host.model(cfg)
            try:
                for i, w in enumerate(_weights(shape, mode)):
                    m.set_weight(i, w)
                st = _stream(shape, first)
                m.decode_begin(st)
                for n in range(1, n_last + 1):
                    m.decode_step(n, graph)
                    if n in checks:
                        lg = m.logits(st[:n], n - 1)            # (the fused step again: the same row, the same bytes)
                        out[n][0][first] = (m.decode_result(n), _digest(lg))
                        out[n][1][first] = lg
            finally:
                m.close()
        else:
            b = host.batch(cfg, S)
            try:
                for i, w in enumerate(_weights(shape, mode)):
                    b.set_weight(i, w)
                for j, q in enumerate(qs):
                    b.decode_begin(j, _stream(shape, q))
                for n in range(1, n_last + 1):
                    b.decode_step(n, graph)
                    if n in checks:
                        for j, q in enumerate(qs):
                            lg = b.logits(j)
                            out[n][0][q] = (b.decode_result(j, n), _digest(lg))
                            if q in SEAMS or j == S - 1:
                                out[n][1][q] = lg
            finally:
                b.close()
    finally:
        hip.set_ffn_streamed(True)
    _DEV[key] = out
    return out


def oracle_run(oracle, shape, mode, q, n_last, checks):
    key = (shape, mode, q, n_last)
    if key not in _ORC:
        ocfg = ocfg_of(shape, mode)
        om = oracle.model(ocfg)
        try:
            for i, w in enumerate(_weights(shape, mode)):
                om.set_weight(i, w)
            st = _stream(shape, q)
            got = {}
            for n in range(1, n_last + 1):
                lg = om.logits(st[:n], n - 1)
                if n in checks:
                    got[n] = lg
        finally:
            om.close()
        _ORC[key] = got
    return _ORC[key]


def watched(S):
    """the first and last sequence, and both sides of every lane seam (63 / 64, 127 / 128) the batch has"""
    return sorted({0, S - 1} | {q for q in (63, 64, 127, 128) if q < S})


def hold_to_oracle(hip, oracle, shape, mode, S, n_last, checks):
    run = device_run(hip, shape, mode, S, n_last=n_last, checks=checks)
    worst = [0.0, 0.0]
    for q in watched(S):
        want_all = oracle_run(oracle, shape, mode, q, n_last, checks)
        for n in checks:
            gid, _ = run[n][0][q]
            glog, want = run[n][1][q], want_all[n]
            assert np.isfinite(glog).all(), (shape, mode, S, q, n)
            std = float(want.std())
            rms, mx = check_logits(mode, glog, want, std)
            worst = [max(worst[0], rms), max(worst[1], mx)]
            assert gid == int(np.argmax(glog)), (shape, mode, S, q, n)        # the device argmax is the argmax of these logits
            top2 = np.sort(want)[-2:]
            if mode == "f16" and top2[1] - top2[0] > 0.03 * max(std / 0.91, 1.0):
                assert gid == int(np.argmax(want)), (shape, mode, S, q, n)
    return worst


def same_bits(a, b, qs, what):
    """two device runs agree on sequences qs at every check: ids and logits bit for bit"""
    for n in a:
        for q in qs:
            ia, da = a[n][0][q]
            ib, db = b[n][0][q]
            diff = ""
            if q in a[n][1] and q in b[n][1]:
                diff = float(np.abs(a[n][1][q] - b[n][1][q]).max())
            assert ia == ib and da == db, (what, "sequence", q, "step", n, "max |dlogit|", diff)


SHAPE_MODES = [(s, m) for s in SHAPES for m in MODE]
WIDE = [(s, m) for s, m in SHAPE_MODES if (s, m) != ("D", "q8")]        # (decoder_create: q8 at 16+ sequences wants n_ffn <= 5632)


# ---------------------------------------------------------------- a. against the oracle

@pytest.mark.oracle_parity
@pytest.mark.parametrize("shape,mode,S", [(s, m, S) for s, m in SHAPE_MODES for S in (1, 8)] +
                         [(s, m, S) for s, m in WIDE for S in (64, lane_batch(s))])
def test_widths_against_the_oracle(hip, oracle, shape, mode, S):
    hold_to_oracle(hip, oracle, shape, mode, S, SHORT, CHECKS)


# one shape per dtype across the 256-position chunk boundary: f16 with planes and per-head attention, q8 with the streamed
# gate|up in a lane of 128 rows, q4 in three lanes of 64 with the ragged lm_head
@pytest.mark.oracle_parity
@pytest.mark.parametrize("shape,mode,S", [("C", "f16", 64), ("E", "q8", 128), ("B", "q4", 192)])
def test_widths_long_context_against_the_oracle(hip, oracle, shape, mode, S):
    worst = hold_to_oracle(hip, oracle, shape, mode, S, LONG, LONG_CHECKS)
    print(f"{mode} shape {shape} S={S} to n={LONG}: worst rms {worst[0]:.4g} max {worst[1]:.4g} against the oracle")


# ---------------------------------------------------------------- b. bit identity where it is promised

@pytest.mark.parametrize("shape,mode", SHAPE_MODES)
def test_eight_sequences_equal_the_single_sequence_decoder(hip, shape, mode):
    many = device_run(hip, shape, mode, 8)
    for q in range(8):
        same_bits(many, device_run(hip, shape, mode, 1, first=q), [q], (shape, mode, "8 sequences vs single"))


@pytest.mark.parametrize("S", [64, 128])
@pytest.mark.parametrize("shape,mode", WIDE)
def test_streamed_switch_changes_no_bit(hip, shape, mode, S):
    """gten_hip_set_ffn_streamed is a launch-structure switch only (include/gten_hip.h) -- at every width, not only where the
    streamed kernels are taken"""
    same_bits(device_run(hip, shape, mode, S), device_run(hip, shape, mode, S, streamed=False), range(S), (shape, mode, S, "streamed vs slab"))


@pytest.mark.parametrize("shape,mode", WIDE)
def test_lanes_equal_separate_64_sequence_decoders(hip, shape, mode):
    S = lane_batch(shape)
    big = device_run(hip, shape, mode, S)
    for first in range(0, S, 64):
        same_bits(big, device_run(hip, shape, mode, 64, first=first), range(first, first + 64), (shape, mode, S, "lanes vs 64 from", first))


@pytest.mark.parametrize("shape,mode", WIDE)
def test_graph_replay_equals_eager_launches(hip, shape, mode):
    same_bits(device_run(hip, shape, mode, 64), device_run(hip, shape, mode, 64, graph=False), range(64), (shape, mode, "graph vs eager"))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_f16_wide_batches_agree_where_they_split_alike(hip, shape):
    """gten_hip_set_wx_planes's promise as narrowed: f16 decoders of 16, 32, 48 and 64 sequences agree bit for bit on the
    sequences they share wherever their lanes split gate | up and q | k | v into the same K planes (f16_split)"""
    groups = {}
    for S in (16, 32, 48, 64):
        groups.setdefault(f16_split(shape, S), []).append(S)
    assert any(48 in g and 64 in g for g in groups.values())            # (never vacuous: 48 and 64 split alike at every width)
    for sizes in groups.values():
        for S in sizes[1:]:
            same_bits(device_run(hip, shape, "f16", sizes[0]), device_run(hip, shape, "f16", S), range(16), (shape, "f16", sizes[0], "vs", S))


# ---------------------------------------------------------------- c. the branches of SHAPES did run

@pytest.mark.parametrize("S", [64, 128])
@pytest.mark.parametrize("shape,mode", WIDE)
def test_gate_up_takes_the_expected_form(hip, shape, mode, S):
    host = load_package().load_host()
    cfg = host_cfg(ocfg_of(shape, mode))
    hip.prof_family_index("decode_gemv_gateup")                         # (the family exists under this name)
    b = host.batch(cfg, S)
    try:
        for i, w in enumerate(_weights(shape, mode)):
            b.set_weight(i, w)
        for q in range(S):
            b.decode_begin(q, _stream(shape, q))
        for n in range(1, 3):
            b.decode_step(n, True)
        hip.prof_enable(1)
        try:
            b.decode_step(3, False)
            got = hip.prof_read().get("decode_gemv_gateup", (0, 0.0))[0]
        finally:
            hip.prof_enable(0)
        H, KV = SHAPES[shape][2:4]
        assert b.kv_info()[0] == (H // KV in (1, 2, 4, 8)), (shape, mode, S)      # head-major shadows: the q|k|v planes' premise
    finally:
        b.close()
    assert got == gate_up_launches(shape, mode, S), (shape, mode, S, got, gate_up_launches(shape, mode, S))


def test_q8_wide_decoder_past_its_weight_slab_is_refused_at_creation(hip):
    """decoder_create takes n_ffn up to 6144, but a q8 down-projection workgroup of the wide step holds K <= 5632 (MMV_MAXP):
    a 16-sequence q8 decoder of shape D is refused when it is created, with the limit in the message -- not at its first step,
    after the launches before the down projection.  The host library ends the process on an error, so a child process runs it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "\n".join([
        "import sys",
        f"sys.path[:0] = [{root!r}, {os.path.join(root, 'tests')!r}]",
        "from __graft_entry__ import load_package",
        "import test_decode_widths_gpu as t",
        "from test_model_gpu import host_cfg",
        "pkg = load_package()",
        "pkg.hipabi.load(0)",
        "b = pkg.load_host().batch(host_cfg(t.ocfg_of('D', 'q8')), 16)",
        "for i, w in enumerate(t._weights('D', 'q8')):",
        "    b.set_weight(i, w)",
        "for q in range(16):",
        "    b.decode_begin(q, t._stream('D', q))",
        "b.decode_step(1, False)",
        "print('STEPPED')",
    ])
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "STEPPED" not in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "decoder_create: q8 weights with n_seq >= 16 want n_ffn <= 5632" in r.stderr, r.stderr[-2000:]
