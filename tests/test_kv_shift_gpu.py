"""-m gpu: the context shift operator on plain device buffers (include/gten_hip_shift.h).

gten_hip_kv_shift is held to tests/shift_ref.py byte for byte: the half swaps in numpy, the oracle's rotary_emb at row `drop`, the
swaps back; V is row copies.  Canary rows behind n, canary pitch padding and the kept rows must come back untouched.  A last test
does not rest on the definition's own direction: attention over shifted caches against float64 from the pre-RoPE values."""
import numpy as np
import pytest

import shift_ref as ref
from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from helpers import F16, Q8

pytestmark = pytest.mark.gpu

GEOMS = [(64, 128), (64, 256), (32, 64)]                 # (d_head, kv_dim)
SHAPES = [(3, 0, 1), (3, 1, 1), (17, 0, 16), (17, 1, 3), (300, 16, 100), (300, 16, 200), (40, 4, 36), (2048, 0, 2047), (2048, 5, 1)]
TAIL = 3                                                 # canary rows behind n


def dev(hip, a):
    return load_package().hipabi.DeviceBuffer.from_numpy(hip, np.ascontiguousarray(a))


def make_cache(oracle, rng, dtype, kv_dim, n, pad, zero_head_rows=()):
    """uint8 [n + TAIL][row_bytes + pad]: rows [0, n) hold quantised values, everything else (tail rows, padding) random canary bytes"""
    rb = hip_row_bytes(dtype, kv_dim)
    buf = rng.integers(0, 256, (n + TAIL, rb + pad), dtype=np.uint8)
    x = (rng.standard_normal((n, kv_dim)) * rng.choice([0.05, 1.0, 30.0], (n, 1))).astype(np.float32)
    for r in zero_head_rows:
        x[r, :64] = 0.0
    buf[:n, :rb] = oracle.quantize_rows(x, dtype)
    return buf


def hip_row_bytes(dtype, cols):
    return cols * 2 if dtype == F16 else (cols // 32) * 34


def run_items(hip, oracle, dtype, d_head, kv_dim, pad, caches, shapes, one_call=True):
    """shift every (k, v) of `caches` by its shape on the device; returns the downloaded (k, v) pairs"""
    pitch = hip_row_bytes(dtype, kv_dim) + pad
    bufs = [(dev(hip, k), dev(hip, v)) for k, v in caches]
    items = [(bk.ptr, bv.ptr, n, keep, drop) for (bk, bv), (n, keep, drop) in zip(bufs, shapes)]
    if one_call:
        hip.kv_shift(items, dtype, pitch, kv_dim, d_head)
    else:
        for it in items:
            hip.kv_shift([it], dtype, pitch, kv_dim, d_head)
    hip.sync()
    out = [(bk.download(np.uint8, caches[i][0].shape), bv.download(np.uint8, caches[i][1].shape)) for i, (bk, bv) in enumerate(bufs)]
    for bk, bv in bufs:
        bk.free()
        bv.free()
    return out


def check_against_ref(oracle, dtype, d_head, kv_dim, k, v, got, shape):
    n, keep, drop = shape
    rk, rv = ref.shift_ref(oracle, k, v, dtype, kv_dim, d_head, n, keep, drop)
    m = n - keep - drop
    rb = hip_row_bytes(dtype, kv_dim)
    for name, g, r, old in (("K", got[0], rk, k), ("V", got[1], rv, v)):
        assert np.array_equal(g[:keep], old[:keep]), f"{name}: a kept row changed"
        assert np.array_equal(g[keep + max(m, 0):], old[keep + max(m, 0):]), f"{name}: a row behind the moved ones changed (canaries included)"
        assert np.array_equal(g[:, rb:], old[:, rb:]), f"{name}: pitch padding changed"
        bad = np.nonzero((g != r).any(axis=1))[0]
        assert bad.size == 0, f"{name}: {bad.size} rows differ from the reference, first {bad[:4]}"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_keep%d_drop%d" % s)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "dh%d_kv%d" % g)
@pytest.mark.parametrize("dtype", [Q8, F16], ids=["q8", "f16"])
def test_shift_equals_reference(hip, oracle, dtype, geom, shape):
    d_head, kv_dim = geom
    rng = np.random.default_rng(hash((dtype, geom, shape)) & 0xffff)
    n = shape[0]
    k, v = make_cache(oracle, rng, dtype, kv_dim, n, 16), make_cache(oracle, rng, dtype, kv_dim, n, 16)
    (got,) = run_items(hip, oracle, dtype, d_head, kv_dim, 16, [(k, v)], [shape])
    check_against_ref(oracle, dtype, d_head, kv_dim, k, v, got, shape)
    if shape == (40, 4, 36):                             # m = 0: not one byte written
        assert np.array_equal(got[0], k) and np.array_equal(got[1], v)


@pytest.mark.parametrize("pad", [0, 6, 16])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "dh%d_kv%d" % g)
@pytest.mark.parametrize("dtype", [Q8, F16], ids=["q8", "f16"])
def test_every_piece_width_of_v(hip, oracle, dtype, geom, pad):
    """V moves in 16-, 4- or 2-byte pieces by what the pitch and the row allow: pad 6 leaves only 2-byte pieces"""
    d_head, kv_dim = geom
    rng = np.random.default_rng(pad)
    shape = (21, 2, 5)
    k, v = make_cache(oracle, rng, dtype, kv_dim, shape[0], pad), make_cache(oracle, rng, dtype, kv_dim, shape[0], pad)
    (got,) = run_items(hip, oracle, dtype, d_head, kv_dim, pad, [(k, v)], [shape])
    check_against_ref(oracle, dtype, d_head, kv_dim, k, v, got, shape)


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "dh%d_kv%d" % g)
def test_all_zero_q8_head(hip, oracle, geom):
    """a Q8 head that is all zero (delta 0) comes back as the reference's bytes, and those hold no NaN"""
    d_head, kv_dim = geom
    rng = np.random.default_rng(5)
    shape = (12, 1, 2)
    k = make_cache(oracle, rng, Q8, kv_dim, shape[0], 16, zero_head_rows=range(0, 12, 2))
    v = make_cache(oracle, rng, Q8, kv_dim, shape[0], 16)
    assert not k[4, :34].any()                           # (quants and delta of the first block of a zeroed row)
    (got,) = run_items(hip, oracle, Q8, d_head, kv_dim, 16, [(k, v)], [shape])
    check_against_ref(oracle, Q8, d_head, kv_dim, k, v, got, shape)
    rb = hip_row_bytes(Q8, kv_dim)
    vals = oracle.dequantize_rows(got[0][:10, :rb], Q8, kv_dim)
    assert np.isfinite(vals).all()
    assert got[0][1, :34].any() and not got[0][2, :34].any()             # row 1 = unrot(old row 3), row 2 = unrot(old row 4), the zeroed one


@pytest.mark.parametrize("dtype", [Q8, F16], ids=["q8", "f16"])
def test_six_items_in_one_call_equal_six_calls(hip, oracle, dtype):
    """three "sequences" x two "layers", six different shifts: one launch gives what the six single calls give, and the reference"""
    d_head, kv_dim = 64, 128
    rng = np.random.default_rng(11)
    shapes = [(17, 1, 3), (64, 0, 5), (90, 16, 60), (33, 4, 29), (70, 2, 1), (5, 0, 4)]
    caches = [(make_cache(oracle, rng, dtype, kv_dim, s[0], 16), make_cache(oracle, rng, dtype, kv_dim, s[0], 16)) for s in shapes]
    one = run_items(hip, oracle, dtype, d_head, kv_dim, 16, caches, shapes, one_call=True)
    six = run_items(hip, oracle, dtype, d_head, kv_dim, 16, caches, shapes, one_call=False)
    for (k, v), a, b, s in zip(caches, one, six, shapes):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        check_against_ref(oracle, dtype, d_head, kv_dim, k, v, a, s)


def test_invalid_items_are_refused_and_nothing_is_written(hip, oracle):
    d_head, kv_dim, dtype = 64, 128, Q8
    rng = np.random.default_rng(3)
    pitch = hip_row_bytes(dtype, kv_dim) + 16
    k, v = make_cache(oracle, rng, dtype, kv_dim, 40, 16), make_cache(oracle, rng, dtype, kv_dim, 40, 16)
    bk, bv = dev(hip, k), dev(hip, v)
    good = (bk.ptr, bv.ptr, 40, 2, 5)
    cases = [((bk.ptr, bv.ptr, 40, 2, 0), "drop 0"), ((bk.ptr, bv.ptr, 40, 30, 11), "exceed"), ((bk.ptr, bv.ptr, 2049, 0, 1), "2049 rows"),
             ((bk.ptr, bv.ptr, 40, -1, 2), "negative")]
    for bad, text in cases:
        # the valid item comes first: the refusal is all-or-nothing
        assert hip.kv_shift_rc([good, bad], dtype, pitch, kv_dim, d_head) != 0
        assert text in hip._err().decode(), (text, hip._err().decode())
    assert hip.kv_shift_rc([good], dtype, hip_row_bytes(dtype, 96), 96, 48) != 0
    assert "d_head 48" in hip._err().decode()
    assert hip.kv_shift_rc([good], 2, pitch, kv_dim, d_head) != 0           # f32 is no activation dtype of a cache
    assert hip.kv_shift_rc([], dtype, pitch, kv_dim, d_head) != 0
    hip.sync()
    assert np.array_equal(bk.download(np.uint8, k.shape), k) and np.array_equal(bv.download(np.uint8, v.shape), v)
    hip.kv_shift([good], dtype, pitch, kv_dim, d_head)                      # ... and the valid item alone goes through
    hip.sync()
    check_against_ref(oracle, dtype, d_head, kv_dim, k, v, (bk.download(np.uint8, k.shape), bv.download(np.uint8, v.shape)), good[2:])


# ------------------------------------------------------------------------------------------------ the direction of the rotation

def rope64(x, pos, d_head):
    """float64 rotate-half RoPE of [rows][heads * d_head] at positions pos[rows]"""
    rows, d = x.shape
    half = d_head // 2
    th = np.asarray(pos, np.float64)[:, None] * (10000.0 ** (-(2.0 * np.arange(half) / d_head)))[None, :]
    c, s = np.cos(th)[:, None, :], np.sin(th)[:, None, :]
    h = x.reshape(rows, d // d_head, 2, half)
    out = np.empty_like(h)
    out[:, :, 0] = h[:, :, 0] * c - h[:, :, 1] * s
    out[:, :, 1] = h[:, :, 0] * s + h[:, :, 1] * c
    return out.reshape(rows, d)


def attn_errors(hip, oracle, dtype):
    """(error of attention over shifted caches, error over the unshifted rows) of one query, both against float64 from pre-RoPE values"""
    d_head, n_heads, n_kv = 64, 4, 2
    kv_dim, q_dim = n_kv * d_head, n_heads * d_head
    n, d = 96, 37
    n2 = n - d
    rng = np.random.default_rng(17)
    deq = lambda b, w: oracle.dequantize_rows(b, dtype, w).astype(np.float64)                       # noqa: E731
    k_st = oracle.quantize_rows(rng.standard_normal((n, kv_dim)).astype(np.float32), dtype)         # pre-RoPE, in storage
    v_st = oracle.quantize_rows(rng.standard_normal((n, kv_dim)).astype(np.float32), dtype)
    q_row = oracle.quantize_rows(rng.standard_normal((1, q_dim)).astype(np.float32), dtype)
    k_pre, v_val, q_pre = deq(k_st, kv_dim), deq(v_st, kv_dim), deq(q_row, q_dim)
    # float64: the query at distance n - 1 - i from row i, i in [d, n) -- only differences of positions enter
    qr = rope64(q_pre, [n - 1], d_head).reshape(n_heads, d_head)
    kr = rope64(k_pre[d:], np.arange(d, n), d_head).reshape(n2, n_kv, d_head)
    want = np.empty((n_heads, d_head))
    for h in range(n_heads):
        g = h // (n_heads // n_kv)
        s = kr[:, g] @ qr[h] / np.sqrt(d_head)
        p = np.exp(s - s.max())
        want[h] = (p / p.sum()) @ v_val[d:].reshape(n2, n_kv, d_head)[:, g]
    want = want.reshape(-1)
    # the caches as a model leaves them: K rotated at its row's position
    bk, bv = dev(hip, k_st), dev(hip, v_st)
    hip.rotary_emb(bk, dtype, n, kv_dim, d_head)

    def query_at(pos, row):
        """q rotated at `pos`, stored at row `row` of a fresh q matrix"""
        qm = np.zeros((n, q_row.shape[1]), np.uint8)
        qm[pos] = q_row[0]
        b = dev(hip, qm)
        hip.rotary_emb(b, dtype, pos + 1, q_dim, d_head, start_pos=pos)
        hip.sync()
        qm2 = np.zeros_like(qm)
        qm2[row] = b.download(np.uint8, qm.shape)[pos]
        b.free()
        return dev(hip, qm2)

    def attend(q, k, v):
        out = hip.alloc(n * q_row.shape[1])
        out.zero()
        hip.qkv_attn(q, k, v, out, dtype, n2, n_heads, n_kv, d_head, start_pos=n2 - 1)
        hip.sync()
        got = deq(out.download(np.uint8, (n, q_row.shape[1]))[n2 - 1:n2], q_dim)[0]
        out.free()
        return float(np.abs(got - want).max())

    # (b) the old rows [d, n) as they are, in a buffer of their own, the query at n - 1
    hip.sync()
    old_k = bk.download(np.uint8, k_st.shape)
    bk_b, bv_b = dev(hip, np.concatenate([old_k[d:], old_k[:d]])), dev(hip, np.concatenate([v_st[d:], v_st[:d]]))
    err_unshifted = attend(query_at(n - 1, n2 - 1), bk_b, bv_b)
    # (a) the caches shifted by (0, d), the query at n - 1 - d
    hip.kv_shift([(bk.ptr, bv.ptr, n, 0, d)], dtype, k_st.shape[1], kv_dim, d_head)
    err_shifted = attend(query_at(n2 - 1, n2 - 1), bk, bv)
    return err_shifted, err_unshifted, float(np.abs(want).max())


@pytest.mark.parametrize("dtype", [Q8, F16], ids=["q8", "f16"])
def test_attention_over_shifted_caches_matches_relative_positions(hip, oracle, dtype):
    """One extra rounding to the activation dtype per K element suggests 1.4 to 2 times the unshifted path's error; 3 leaves room and
    still fails a rotation the wrong way round, which is off by the size of the values themselves."""
    err_shifted, err_unshifted, scale = attn_errors(hip, oracle, dtype)
    print(f"attention error vs float64 ({'q8' if dtype == Q8 else 'f16'}): shifted {err_shifted:.3e}, unshifted {err_unshifted:.3e}, "
          f"largest output {scale:.3f}")
    assert err_unshifted > 0
    assert err_shifted <= 3 * err_unshifted
