"""-m gpu: calibrated Q4 loading on the device (include/gten_hip_calib.h, include/gten_host_calib.h): the delta
search against tests/calib_ref.py byte for byte and never worse than the plain quantiser in float64; its refusals; the column
energy against float64; the host flow on a small model."""
import functools

import numpy as np
import pytest

from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from calib_ref import col_energy, convert, search_q4, unpack_stream

pytestmark = pytest.mark.gpu

# (1, 32): one block;  (3, 96): fewer blocks than a wave owns;  (17, 544): a span and a row count that are no multiple of the workgroup's
SHAPES = [(1, 32), (3, 96), (17, 544)]
SEARCH_CASES = [(src, shape, imp) for src in ("f32", "bf16", "f16") for shape in SHAPES for imp in ("none", "positive", "zeros")]


def as_src(w, src):
    """f32 values already rounded to `src` -> the elements as the device takes them"""
    return {"f32": lambda: w, "f16": lambda: w.astype(np.float16), "bf16": lambda: (w.view(np.uint32) >> 16).astype(np.uint16)}[src]()


@functools.lru_cache(maxsize=None)
def search_inputs(src, shape, imp):
    """a Gaussian matrix in the dtype's own values; from five blocks on it carries, in blocks 0..4: all zeros; one large outlier;
    equal magnitudes (ties); amax / 7 beyond f16 (delta0 infinite, kept; an f16 source cannot hold one, there amax = 60000); an
    f16-subnormal delta0.  Importance: none | random positive | random with an all-zero last block span and single zeros"""
    rows, cols = shape
    rng = np.random.default_rng(rows * 4099 + cols)
    w = (rng.standard_normal(shape) * 0.05).astype(np.float32)
    blocks = w.reshape(-1, 32)
    if len(blocks) >= 5:
        blocks[0] = 0
        blocks[1, 13] = 3.0
        blocks[2] = 0.75 * (1 - 2 * (np.arange(32) % 2))
        blocks[3, 7] = 60000.0 if src == "f16" else 5e5
        blocks[4] = rng.integers(-127, 128, 32).astype(np.float32) * 2.0 ** -22
    w = convert._round_to(w, src)
    importance = None if imp == "none" else rng.uniform(0.25, 4.0, cols).astype(np.float32)
    if imp == "zeros":
        importance[::5] = 0
        importance[-32:] = 0
    return w, importance


@functools.lru_cache(maxsize=None)
def device_search(hip, src, shape, imp):
    w, importance = search_inputs(src, shape, imp)
    buf = hip.quantize_weight_search(as_src(w, src), src, *shape, importance)
    got = buf.download()
    buf.free()
    return got


@pytest.mark.parametrize("src, shape, imp", SEARCH_CASES)
def test_search_bytes_are_the_packed_reference(hip, src, shape, imp):
    w, importance = search_inputs(src, shape, imp)
    want_buf = hip.upload_weight(search_q4(w, importance, src), 4, *shape)
    want = want_buf.download()
    want_buf.free()
    got = device_search(hip, src, shape, imp)
    bad = np.flatnonzero(got != want)
    assert got.size == want.size and bad.size == 0, (bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("src, shape, imp", SEARCH_CASES)
def test_search_is_never_worse_than_the_plain_quantiser_in_float64(hip, src, shape, imp):
    """per block, err64(device) <= err64(convert.quantize) * (1 + 2^-18), err64 the weighted squared error in float64.  The slack is
    derived: the kernel compares f32 errors, and each of an error's 32 non-negative terms passes 4 roundings (d * q, the
    difference, the square, the weight) and at most 9 sums (8 in its lane, counting 0 + t, and 2 of the tree, less one), so each
    f32 err is within 14 u of the exact one, u = 2^-24.  A strict f32 comparison can therefore prefer a candidate whose exact
    error is larger by a factor of at most (1 + 14 u) / (1 - 14 u) < 1 + 28 u / (1 - 14 u) < 1 + 2^-18.  Blocks whose bytes equal
    the plain ones are never worse (a non-finite plain delta has no error to compare).  Over the Gaussian (17, 544) matrix the
    summed error is strictly smaller."""
    w, importance = search_inputs(src, shape, imp)
    rows, cols = shape
    nb, nblk = cols // 32, rows * cols // 32
    got = device_search(hip, src, shape, imp)
    stream = np.concatenate([got[nblk * 16:].reshape(nblk, 2), got[:nblk * 16].reshape(nblk, 16)], axis=1)     # packed planes -> blocks
    plain = convert.quantize(w, "q4", src)
    x = w.reshape(rows, nb, 32).astype(np.float64)
    wt = np.broadcast_to((np.ones(cols) if importance is None else importance.astype(np.float64)).reshape(1, nb, 32), x.shape)

    def err64(blocks):
        d, q = unpack_stream(blocks, rows, nb)
        with np.errstate(all="ignore"):
            return (wt * (x - d.astype(np.float64)[..., None] * q) ** 2).sum(axis=2)
    dev, ref = err64(stream), err64(plain)
    same = (stream.reshape(rows, nb, 18) == plain.reshape(rows, nb, 18)).all(axis=2)
    assert (same | (dev <= ref * (1 + 2.0 ** -18))).all(), np.argwhere(~(same | (dev <= ref * (1 + 2.0 ** -18))))[:8]
    if shape == (17, 544):
        fine = np.isfinite(ref)
        assert fine.sum() >= nblk - 1 and dev[fine].sum() < ref[fine].sum()


def test_search_refusals_by_name_and_the_next_call_succeeds(hip):
    Err = load_package().hipabi.GtenHipError
    w, importance = search_inputs("f32", (3, 96), "positive")
    spoiled_w = w.copy()
    spoiled_w[1, 40] = np.nan
    for elements, imp, cols, said in [(spoiled_w, importance, 96, "quantize_weight_search: the source holds a NaN or an infinity"),
                                      (w, np.where(np.arange(96) == 50, np.float32(-1.0), importance), 96, "quantize_weight_search: the importance holds a negative"),
                                      (w, np.where(np.arange(96) == 95, np.float32(np.inf), importance), 96, "quantize_weight_search: the importance holds"),
                                      (w[:, :48], importance[:48], 48, "quantize_weight_search: cols 48 not a multiple")]:
        with pytest.raises(Err, match=said):
            hip.quantize_weight_search(np.ascontiguousarray(elements), "f32", 3, cols, imp)
        hip.quantize_weight_search(w, "f32", 3, 96, importance).free()         # the flags are down again


def q8_rows(x):
    """f32 [n][cols] -> (Q8 row bytes as activations are stored: {f16 delta, int8 x 32} per block, the f32 values they hold)"""
    rows = convert.quantize_q8(x)
    blocks = rows.reshape(len(x), -1, 34)
    d = np.ascontiguousarray(blocks[:, :, :2]).view(np.float16).astype(np.float32)
    return rows, (d * blocks[:, :, 2:].view(np.int8).astype(np.float32)).reshape(x.shape)


@pytest.mark.parametrize("cols", [64, 2048 + 64])
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("adtype", [3, 1])
def test_col_energy_against_float64_and_bit_equal_between_equal_call_sequences(hip, adtype, n_rows, cols):
    """two successive calls into one accumulator, twice: both accumulators hold the same bits and twice the float64 energy within
    1e-12; at 65 rows the rows are a padded, offset view (pitch + 6, base + 2: inside the row contract)"""
    rng = np.random.default_rng(n_rows * 31 + cols)
    x = rng.standard_normal((n_rows, cols)).astype(np.float32)
    data, values = q8_rows(x) if adtype == 3 else (x.astype(np.float16).view(np.uint8), x.astype(np.float16).astype(np.float32))
    rb = data.shape[1]
    pad, off = (6, 2) if n_rows == 65 else (0, 0)
    host = np.zeros((n_rows, rb + pad), np.uint8)
    host[:, :rb] = data
    buf = hip.upload(np.concatenate([np.zeros(off, np.uint8), host.reshape(-1)]))
    accs = [hip.upload(np.zeros(cols, np.float64)) for _ in range(2)]
    for acc in accs:
        for _ in range(2):
            hip.calib_col_energy(buf.view(off), adtype, n_rows, cols, acc, pitch=rb + pad)
    hip.sync()
    got = [acc.download(np.float64) for acc in accs]
    for b in [buf] + accs:
        b.free()
    want = 2 * col_energy(values)
    assert got[0].tobytes() == got[1].tobytes()
    assert (np.abs(got[0] - want) <= 1e-12 * want).all(), np.abs(got[0] / want - 1).max()


def test_the_flow_on_a_small_q4_model(hip):
    pkg = load_package()
    host = pkg.load_host()
    cfg = host.default_config(4, 3)
    cfg.n_vocab, cfg.max_ctx, cfg.n_embd, cfg.n_ffn, cfg.n_layers, cfg.n_heads, cfg.n_kv_heads = 515, 64, 256, 512, 2, 4, 2
    E = cfg.n_embd
    rng = np.random.default_rng(11)
    model = host.model(cfg)
    model.load_synthetic(7)
    texts = [rng.integers(0, cfg.n_vocab, 20).astype(np.int32), rng.integers(0, cfg.n_vocab, 7).astype(np.int32)]      # the block call, the modules
    imp = model.collect_importance(texts)
    assert model.calib_rows() == 27 and sorted(imp) == [1 + 9 * l + k for l in range(2) for k in range(7)]
    for l in range(2):
        vec = [imp[1 + 9 * l + k] for k in range(7)]
        assert all(v.dtype == np.float32 and np.isfinite(v).all() and (v >= 0).all() and v.any() for v in vec)
        assert [v.size for v in vec] == [E, E, E, E, E, E, cfg.n_ffn]
        assert (vec[0] == vec[1]).all() and (vec[0] == vec[2]).all() and (vec[4] == vec[5]).all()

    # layer 0, input of q | k | v: rms_norm(token_embed(ids)) through the operators
    ids = np.concatenate(texts)
    bufs = [hip.upload(model.weight_read(0)), hip.upload(model.weight_read(8)), hip.upload(ids), hip.alloc(27 * hip.row_bytes(3, E)),
            hip.alloc(27 * hip.row_bytes(3, E)), hip.upload(np.zeros(E, np.float64))]
    hip.token_embed(bufs[0], 4, cfg.n_vocab, bufs[2], bufs[3], 3, 27, E)
    hip.rms_norm(bufs[3], 3, bufs[1], bufs[4], 27, E)
    hip.calib_col_energy(bufs[4], 3, 27, E, bufs[5])
    hip.sync()
    want = bufs[5].download(np.float64)
    for b in bufs:
        b.free()
    got = model.calib_read(0, 0)
    assert want.min() > 0 and (np.abs(got - want) <= 1e-6 * want).all(), np.abs(got / want - 1).max()

    # layer 0's linears from f16 elements: with the importance, the search's bytes; without, today's
    Err = pkg.hipabi.GtenHipError
    for i, (r, c, _) in enumerate(cfg.weight_shapes()):
        if not 1 <= i <= 7:
            continue
        w = convert._round_to((rng.standard_normal((r, c)) * 0.05).astype(np.float32), "f16").astype(np.float16)
        for importance, want_buf in ((imp[i], hip.quantize_weight_search(w, "f16", r, c, imp[i])), (None, hip.quantize_weight(w, "f16", 4, r, c))):
            model.set_weight_from(i, w, "f16", importance=importance)
            assert np.array_equal(model.weight_read(i), want_buf.download()), (i, importance is None)
            want_buf.free()
    with pytest.raises(Err, match="embed_tokens"):
        model.set_weight_from(0, np.zeros((cfg.n_vocab, E), np.float16), "f16", importance=np.ones(E, np.float32))
    with pytest.raises(Err, match="importance of 32 values for 256 columns"):
        model.set_weight_from(1, np.zeros((E, E), np.float16), "f16", importance=np.ones(32, np.float32))
    with pytest.raises(Err, match="importance together with lora"):
        model.set_weight_from(1, np.zeros((E, E), np.float16), "f16", lora=(np.zeros((1, E), np.float16), np.zeros((E, 1), np.float16), 1.0),
                              importance=np.ones(E, np.float32))
    model.quant_release()
    model.close()
