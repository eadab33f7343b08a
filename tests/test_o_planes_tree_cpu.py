"""wave_sum's tree over 64 lanes (csrc/gten_dev.h) equals four 16-lane trees combined as (p0 + p1) + (p2 + p3), bit for bit: the
association that k_dec_o_planes (one 16-lane tree per K quarter, a plane each) and its consumer (the gate|up launch, which adds the
planes in that order) rely on to keep the bytes of the one-plane o launch -- csrc/gten_decode_oplanes.h.

The emulation follows the documented steps in numpy float32: quads (xor 1, xor 2), row_half_mirror, row_mirror, row_bcast15 into rows
1 and 3, row_bcast31 into rows 2 and 3 (a row outside a step's mask adds the 0 the DPP move leaves there), lane 63 read."""
import numpy as np

N_VECTORS = 100_000
LANES = np.arange(64)


def _tree16(v):
    """the first four steps, on any number of aligned 16-lane rows along the last axis: every lane ends with its row's sum"""
    lanes = np.arange(v.shape[-1])
    v = v + v[..., lanes ^ 1]
    v = v + v[..., lanes ^ 2]
    v = v + v[..., (lanes & ~7) | (7 - (lanes & 7))]
    return v + v[..., (lanes & ~15) | (15 - (lanes & 15))]


def wave_sum(v):
    assert v.dtype == np.float32 and v.shape[-1] == 64
    v = _tree16(v)
    row = LANES >> 4
    zero = np.float32(0.0)
    b15 = np.where((row == 1) | (row == 3), v[..., np.maximum(row - 1, 0) * 16 + 15], zero)       # row mask 0xA
    v = v + b15
    b31 = np.where(row >= 2, v[..., [31] * 64], zero)                                                # row mask 0xC
    v = v + b31
    return v[..., 63]


def plane_sum(v):
    p = [_tree16(np.ascontiguousarray(v[..., 16 * q: 16 * q + 16])) for q in range(4)]
    for q in range(4):                               # every lane of a row holds the same bits: any one of them may store
        assert np.array_equal(p[q].view(np.uint32), np.repeat(p[q][..., :1], 16, axis=-1).view(np.uint32))
    return (p[0][..., 15] + p[1][..., 15]) + (p[2][..., 15] + p[3][..., 15])


def _vectors():
    rng = np.random.default_rng(20481)
    n = N_VECTORS
    v = rng.standard_normal((n, 64)).astype(np.float32)
    # mixed magnitudes: every lane its own binade over 40 of them, so that the order of the additions shows in the low bits
    third = n // 3
    v[:third] *= np.exp2(rng.integers(-20, 20, (third, 64))).astype(np.float32)
    # zeros and signed zeros sprinkled in; whole rows and whole vectors of them too
    z = rng.random((n, 64))
    v[z < 0.10] = np.float32(0.0)
    v[z > 0.93] = np.float32(-0.0)
    v[0] = np.float32(0.0)
    v[1] = np.float32(-0.0)
    v[2, :16] = np.float32(-0.0); v[2, 48:] = np.float32(0.0)
    v[3, 16:48] = np.float32(-0.0)
    # cancellation: a quarter that is the negative of another
    v[4, 16:32] = -v[4, :16]
    v[5, 48:] = -v[5, :16]
    return v


def test_wave_sum_is_four_quarter_trees_added_in_pairs():
    v = _vectors()
    assert v.shape == (N_VECTORS, 64) and v.dtype == np.float32
    a, b = wave_sum(v), plane_sum(v)
    assert a.dtype == np.float32 and b.dtype == np.float32
    assert np.isfinite(a).all()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # the vectors do tell associations apart: adding the quarters left to right gives other bits somewhere
    p = [_tree16(np.ascontiguousarray(v[:, 16 * q: 16 * q + 16]))[:, 0] for q in range(4)]
    chain = ((p[0] + p[1]) + p[2]) + p[3]
    assert not np.array_equal(a.view(np.uint32), chain.view(np.uint32))


def test_signed_zero_vectors_keep_their_sign():
    v = _vectors()[:4]
    a, b = wave_sum(v), plane_sum(v)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert a[0].view(np.uint32) == 0 and a[1].view(np.uint32) == 0x80000000
