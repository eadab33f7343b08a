"""-m gpu: a LoRA adapter merged into a weight while it is quantised on the device (include/gten_hip_lora.h)
against tests/lora_ref.py and the converter, byte for byte; the cases where the merge is the identity; the refusals; a small
model loaded with the adapter merged on the device and on the host."""
import numpy as np
import pytest

from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from lora_ref import convert, merge

pytestmark = pytest.mark.gpu

CODES = {"f16": 1, "q8": 3, "q4": 4}
# rows 1, 5 | 17 | 33: below, across one and two row tiles of 16;  cols 32 | 544 | 1056: one block, 17 and 33 blocks (a tail group
# alone and behind full groups);  rank 1, 3 | 16 | 17 | 64: inside a chunk of 16, a whole chunk, a chunk tail, the maximum
CASES = [(1, 32, 1, "f32", "q8", "f32"), (5, 544, 3, "bf16", "q4", "bf16"), (17, 1056, 16, "f16", "q8", "f16"),
         (33, 544, 17, "f16", "q4", "f32"), (33, 1056, 64, "bf16", "f16", "f16"), (17, 32, 64, "f32", "f16", "bf16"),
         (5, 1056, 17, "f32", "q4", "f16"), (33, 32, 3, "bf16", "q8", "f32"), (17, 544, 16, "f16", "f16", "bf16")]


def as_src(w, src):
    """f32 values already rounded to `src` -> the elements as the device takes them"""
    return {"f32": lambda: w, "f16": lambda: w.astype(np.float16), "bf16": lambda: (w.view(np.uint32) >> 16).astype(np.uint16)}[src]()


def inputs(rows, cols, rank, src, ab):
    """normal data in the dtypes' own values; from three blocks on, the last block of every row is all zero after the merge and
    the one before it has a subnormal f16 delta (elements of 2^-22 .. 2^-15; A is zero under both)"""
    rng = np.random.default_rng(rows * 4099 + cols * 67 + rank)
    w = (rng.standard_normal((rows, cols)) * 0.05).astype(np.float32)
    a = (rng.standard_normal((rank, cols)) * 0.3).astype(np.float32)
    b = (rng.standard_normal((rows, rank)) * 0.1).astype(np.float32)
    if cols >= 96:
        a[:, -64:] = 0
        w[:, -32:] = 0
        w[:, -64:-32] = rng.integers(-127, 128, (rows, 32)).astype(np.float32) * 2.0 ** -22
    return convert._round_to(w, src), convert._round_to(a, ab), convert._round_to(b, ab)


def device_bytes(hip, w, src, a, b, ab, scale, dst):
    buf = hip.quantize_weight_lora(as_src(w, src), src, as_src(a, ab), as_src(b, ab), ab, scale, CODES[dst], *w.shape)
    got = buf.download()
    buf.free()
    return got


@pytest.mark.parametrize("rows, cols, rank, src, dst, ab", CASES)
def test_merged_weight_is_pack_of_the_converter_on_the_reference_merge(hip, rows, cols, rank, src, dst, ab):
    w, a, b = inputs(rows, cols, rank, src, ab)
    m = merge(w, a, b, 0.75, src)
    assert np.isfinite(m).all() and (m != w).any()
    want_buf = hip.upload_weight(convert.quantize(m, dst, src), CODES[dst], rows, cols)
    want = want_buf.download()
    want_buf.free()
    got = device_bytes(hip, w, src, a, b, ab, 0.75, dst)
    bad = np.flatnonzero(got != want)
    assert got.size == want.size and bad.size == 0, (bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("src, dst", [("f32", "q4"), ("bf16", "q8"), ("f16", "f16")])
def test_zero_scale_and_zero_b_give_the_unmerged_bytes(hip, src, dst):
    """on a source without negative zeros (w + 0 turns -0 into +0, which an f16 destination would show)"""
    w, a, b = inputs(17, 544, 3, src, "f16")
    w[w == 0] = 0.0
    plain = hip.quantize_weight(as_src(w, src), src, CODES[dst], 17, 544)
    want = plain.download()
    plain.free()
    assert np.array_equal(device_bytes(hip, w, src, a, b, "f16", 0.0, dst), want)
    assert np.array_equal(device_bytes(hip, w, src, a, np.zeros_like(b), "f16", 2.0, dst), want)


@pytest.mark.parametrize("dst", ["q8", "q4", "f16"])
def test_non_finite_merges_fail_by_name_and_the_next_call_succeeds(hip, dst):
    Err = load_package().hipabi.GtenHipError
    w, a, b = inputs(17, 544, 3, "f16", "f32")
    spoiled = [(w, np.where(np.arange(a.size).reshape(a.shape) == 700, np.float32(np.nan), a), b),      # a NaN in A
               (w, a, np.where(np.arange(b.size).reshape(b.shape) == 49, np.float32(np.inf), b)),       # an infinity in B
               (np.full_like(w, 60000.0), np.full_like(a, 32.0), np.full_like(b, 64.0))]                # 60000 + 6144: beyond f16
    for w_, a_, b_ in spoiled:
        with pytest.raises(Err, match="quantize_weight_lora.*NaN or an infinity"):
            device_bytes(hip, w_, "f16", a_, b_, "f32", 1.0, dst)
        assert device_bytes(hip, w, "f16", a, b, "f32", 1.0, dst).size         # the flag is down again


def test_refusals_before_any_launch(hip):
    Err = load_package().hipabi.GtenHipError
    w, a, b = inputs(5, 544, 3, "f16", "f16")
    hip.prof_enable(True)
    launches = hip.prof_read().get("pack_weight", (0, 0.0))[0]
    for rank in (0, 65):
        with pytest.raises(Err, match=f"quantize_weight_lora: rank {rank}"):
            device_bytes(hip, w, "f16", np.zeros((rank, 544), np.float32), np.zeros((5, rank), np.float32), "f32", 1.0, "q4")
    for scale in (np.inf, np.nan):
        with pytest.raises(Err, match="quantize_weight_lora: the scale"):
            device_bytes(hip, w, "f16", a, b, "f16", scale, "q4")
    bufs = [hip.upload(as_src(v, "f16")) for v in (w, a, b)] + [hip.alloc(5 * hip.row_bytes(4, 544))]
    rc = hip.quantize_weight_lora_rc(bufs[0], "f16", 5, 512, bufs[1].view(2), bufs[2], 3, "f16", 1.0, 4, bufs[3])
    said = hip.last_error()
    for buf in bufs:
        buf.free()
    assert rc != 0 and "quantize_weight_lora: A and B must be 16-byte aligned" in said
    assert hip.prof_read().get("pack_weight", (0, 0.0))[0] == launches
    hip.prof_enable(False)


@pytest.mark.parametrize("wd", ["f16", "q8", "q4"])
def test_a_model_loaded_with_the_adapter_is_the_model_of_the_merged_weights(hip, wd):
    pkg = load_package()
    host = pkg.load_host()
    cfg = host.default_config(CODES[wd], 1 if wd == "f16" else 3)
    cfg.n_vocab, cfg.max_ctx, cfg.n_embd, cfg.n_ffn, cfg.n_layers, cfg.n_heads, cfg.n_kv_heads = 515, 64, 256, 512, 2, 4, 2
    rng = np.random.default_rng(5)
    one, two = host.model(cfg), host.model(cfg)
    last = one.n_weights() - 1
    for i, (r, c, _) in enumerate(cfg.weight_shapes()):
        w = convert._round_to((rng.standard_normal((r, c)) * (0.05 if r > 1 else 1.0)).astype(np.float32), "f16")
        if 0 < i < last - 1 and (i - 1) % 9 < 7:
            a = convert._round_to((rng.standard_normal((8, c)) * 0.3).astype(np.float32), "bf16")
            b = convert._round_to((rng.standard_normal((r, 8)) * 0.1).astype(np.float32), "bf16")
            one.set_weight_from(i, merge(w, a, b, 2.0, "f16").astype(np.float16), "f16")
            two.set_weight_from(i, w.astype(np.float16), "f16", lora=(as_src(a, "bf16"), as_src(b, "bf16"), 2.0))
        else:
            one.set_weight_from(i, w.astype(np.float16), "f16")
            two.set_weight_from(i, w.astype(np.float16), "f16")
            if r > 1:                                  # embed_tokens and lm_head: refused by name
                with pytest.raises(pkg.hipabi.GtenHipError, match="embed_tokens" if i == 0 else "lm_head"):
                    two.set_weight_from(i, w.astype(np.float16), "f16", lora=(np.zeros((8, c), np.float16), np.zeros((r, 8), np.float16), 2.0))
    for i in range(one.n_weights()):
        assert np.array_equal(one.weight_read(i), two.weight_read(i)), i
    prompt = rng.integers(0, cfg.n_vocab, 20).astype(np.int32)
    logits = [(m.logits(prompt, 0), m.logits(np.append(prompt, np.int32(7)), 20)) for m in (one, two)]     # the prompt, then one decode step
    one.close()
    two.close()
    for la, lb in zip(*logits):
        assert np.isfinite(la).all() and la.std() > 0 and la.tobytes() == lb.tobytes()
