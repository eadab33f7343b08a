"""-m gpu: FP8 (E4M3) head-major K / V shadows of the f16 wide decoders.  R against its NumPy restatement, the shadow
through import and append, k_dec_attn_hm_fp8 against the f16 kernel on rows rounded by R (EQUALITY of logits bytes), a shared prefix."""
import numpy as np
import pytest

import kv_fp8_ref as ref
from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from helpers import F16, Q4, Q8, tiny_config
from test_model_gpu import host_cfg

pytestmark = pytest.mark.gpu


def make_batch(hip, cfg, n_seq, fp8, seed=777):
    host = load_package().load_host()
    hip.set_kv_shadow_fp8(fp8)
    try:
        b = host.batch(cfg, n_seq)
        for i in range(len(cfg.weight_shapes())):
            b.set_weight(i, host.synth_weight(cfg, seed, i))
        b.decode_begin(0, host.synthetic_tokens(4, seed=1, n_vocab=cfg.n_vocab))     # (creates the shared decoder under the switch)
    finally:
        hip.set_kv_shadow_fp8(False)
    return host, b


@pytest.mark.parametrize("pad,offset", [(0, 0), (30, 6)])
def test_round_operator_is_the_restatement_and_idempotent(hip, pad, offset):
    """all 65 536 f16 patterns as 64 rows of 1024 elements, dense and as a padded, offset view whose padding must come back untouched"""
    rows = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.uint8).reshape(64, 2048)
    rb, pitch = 2048, 2048 + pad
    host_img = np.full(offset + 64 * pitch, 0xA5, np.uint8)
    host_img[offset:].reshape(64, pitch)[:, :rb] = rows
    buf = hip.upload(host_img)
    want = ref.round_rows(rows)
    for _ in range(2):                                            # applying it twice equals applying it once
        hip.kv_round_fp8(buf.view(offset), 64, rb, pitch)
        got = buf.download()
        assert np.array_equal(got[offset:].reshape(64, pitch)[:, :rb], want)
        untouched = np.ones(len(got), bool)
        untouched[offset:].reshape(64, pitch)[:, :rb] = False
        assert (got[untouched] == 0xA5).all()
    assert hip.kv_round_fp8_rc(buf.view(1), 1, rb, pitch) != 0 and hip.kv_round_fp8_rc(buf, 1, rb, rb + 1) != 0 and hip.kv_round_fp8_rc(buf, 1, rb - 1, pitch) != 0


def test_shadow_content_through_append_and_import(hip):
    """the shadow built by 290 appends reads back as R of the cache rows; one row rewritten by a library copy forces a re-import"""
    cfg = host_cfg(tiny_config(F16, F16, n_embd=512, n_heads=8, n_kv_heads=2, max_ctx=576, n_layers=2))
    host, b = make_batch(hip, cfg, 16, True)
    assert b.kv_shadow_info()[:2] == (8, 16384)
    N, held = 290, (3, 15)
    for q in range(16):
        b.decode_begin(q, host.synthetic_tokens(N + 1, seed=300 + q, n_vocab=cfg.n_vocab))
    for n in range(1, N + 1):
        b.decode_step(n, True)

    def check(n_rows):
        for q in held:
            for layer in range(2):
                rows, shadow = b.kv_read(q, layer, 0, n_rows), b.kv_shadow_read_fp8(q, layer, n_rows)
                for kv in range(2):
                    assert np.array_equal(shadow[kv], ref.round_rows(rows[kv])), (q, layer, kv)
                    assert not np.array_equal(shadow[kv], rows[kv])      # (R did change the rows: the comparison is not vacuous)
    check(N)
    imports = b.kv_info()[1]
    k_rows, _, pitch = b.kv_rows(held[0], 1)
    rb, tmp = b.kv_row_bytes(), hip.alloc(1024)
    hip.copy_ranges([(tmp.ptr, k_rows + 100 * pitch, rb)])
    hip.copy_ranges([(k_rows + 100 * pitch, tmp.ptr, rb)])
    b.decode_step(N + 1, True)
    assert b.kv_info()[1] == imports + 1
    check(N + 1)
    b.close()
    _, b = make_batch(hip, host_cfg(tiny_config(Q4, Q8, n_heads=4, n_kv_heads=2, max_ctx=320, n_layers=1)), 16, True)
    assert b.kv_shadow_info()[:2] == (8, 17408)                  # Q8 activations keep their Q8 shadows under the switch
    b.close()


@pytest.mark.parametrize("heads,kv,n_seq,N", [(8, 1, 16, 290), (8, 2, 32, 290), (4, 2, 16, 290), (4, 4, 16, 290), (8, 2, 16, 530)])
def test_fp8_kernel_is_the_f16_kernel_on_rounded_rows(hip, heads, kv, n_seq, N):
    """decoder A under the switch against decoder B on f16 shadows whose rows [0, n - 1) are rounded by R before every step n"""
    cfg = host_cfg(tiny_config(F16, F16, n_embd=64 * heads, n_heads=heads, n_kv_heads=kv, max_ctx=576, n_layers=2))
    probes = (1, 2, 16, 17, 33, 255, 256, 257, 258, 290) + ((512, 513, 514, 530) if N > 290 else ())
    held = (0, 1, n_seq // 2, n_seq - 1)
    snaps = []
    for fp8 in (True, False):
        host, b = make_batch(hip, cfg, n_seq, fp8)
        assert b.kv_shadow_info()[:2] == ((8, 16384) if fp8 else (16, 32768))
        for q in range(n_seq):
            b.decode_begin(q, host.synthetic_tokens(N, seed=900 + q, n_vocab=cfg.n_vocab))
        snap = {}
        for n in range(1, N + 1):
            if not fp8 and n > 1:
                for q in range(n_seq):
                    b.kv_round_fp8(q, n - 1)
            b.decode_step(n, True)
            if n in probes:
                snap[n] = [(b.decode_result(q, n), b.logits(q).copy()) for q in held]
        snaps.append(snap)
        b.close()
    for n in probes:
        for (ia, la), (ib, lb), q in zip(snaps[0][n], snaps[1][n], held):
            assert np.isfinite(la).all() and ia == ib and np.array_equal(la, lb), (q, n, float(np.abs(la - lb).max()))


@pytest.mark.parametrize("which", [0, 1])
def test_shared_prefix_under_the_switch(hip, which):
    """a prefix of 270 ids at index 0 (k_dec_attn_hm_fp8_pfx) or 1 (the table form, _pfxn), 16 slots: sharing on is sharing off, byte for byte"""
    cfg = host_cfg(tiny_config(F16, F16, n_heads=4, n_kv_heads=2, n_layers=2, max_ctx=768))
    host, b = make_batch(hip, cfg, 16, True)
    toks = lambda n, seed: [int(t) for t in host.synthetic_tokens(n, seed=seed, n_vocab=cfg.n_vocab)]
    prefix = toks(270, 41)
    prompts = [prefix + toks(16 + 3 * i, 200 + i) for i in range(7)] + [toks(300, 77)]
    steps, out = 20, []
    for on in (False, True):
        host.set_prefix_decode_shared(on)
        try:
            b.set_prefix_at(which, None)
            b.set_prefix_at(which, prefix)
            lg = b.prefill_many(list(range(len(prompts))), prompts)
            streams = [p + toks(steps, 5000 + q) for q, p in enumerate(prompts)]
            for q in range(16):
                b.decode_begin(q, streams[q] if q < len(prompts) else toks(steps + 1, 6000 + q))
            ids = []
            for t in range(1, steps + 1):
                ns = [len(p) + t for p in prompts] + [t] * (16 - len(prompts))
                b.decode_step_ragged(ns, use_graph=(t % 2 == 0))
                ids.append([b.decode_result(q, ns[q]) for q in range(len(prompts))])
            out.append((lg, ids, np.stack([b.logits(q) for q in range(len(prompts))]), [b.prefix_decode_info(q)[1] for q in range(len(prompts))]))
        finally:
            host.set_prefix_decode_shared(None)
    b.close()
    (lg0, ids0, last0, ch0), (lg1, ids1, last1, ch1) = out
    assert ch0 == [0] * 8 and (which != 0 or ch1 == [1] * 7 + [0]), (ch0, ch1)
    assert np.array_equal(lg0, lg1) and ids0 == ids1 and np.array_equal(last0, last1)
