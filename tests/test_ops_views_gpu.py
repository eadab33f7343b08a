"""-m gpu: the operators of include/gten_hip.h on padded, offset row views.

tests/test_ops_gpu.py calls every operator on dense rows at the start of an allocation.  Here the same operators get rows at
a base offset and a pitch (tests/views.py: the geometry classes), inputs and outputs in classes of their own:
  * the result is the oracle's on dense copies of the same rows, with the comparison and tolerance test_ops_gpu.py uses for
    that operator and kernel form -- and the bytes of the dense, aligned call wherever the code establishes that (the same
    kernel; the rms / rope wave kernels against their row kernels; a prompt GEMM fed by either activation conversion);
  * every byte of an output's parent outside the written rows is unchanged (views.outside_untouched), every input's parent
    is the bytes it was;
  * the profiler's launch families show which form ran: a view that lacks the alignment of a wide form leaves it (family
    view_2byte: the shape picks the wide form, the view does not allow it), the control and the 16-byte classes stay;
  * a base or a pitch outside the contract (include/gten_hip.h, "Row views") is refused: nothing launched, nothing written.
"""
import numpy as np
import pytest

import views
from gpu_common import hip  # noqa: F401
from helpers import F16, F32, MODES, Q8, act_rows, compare_rows, rng, row_bytes, weight_rows
from views import CONTROL

pytestmark = pytest.mark.gpu

C16, C8, C4, C2, C2W, C34 = (16, 16), (8, 8), (4, 4), (2, 2), (2, 14), (34, 34)
NARROW = "view_2byte"


class Operand:
    """rows on the device inside a parent full of canaries: .view is what an operator gets, .pitch its pitch"""

    def __init__(self, hip, rows, cls, fill=0xA5):
        self.rows = np.ascontiguousarray(rows).view(np.uint8)
        self.n, self.rb = self.rows.shape
        self.off, pad = cls
        self.pitch = self.rb + pad
        self.before = views.embed(self.rows, self.off, self.pitch, fill)
        self.buf = hip.upload(self.before)
        assert self.buf.ptr % 256 == 0, "base offsets are counted from a 256-aligned address"
        self.view = self.buf.view(views.base(self.off))

    def al(self, a):
        return self.view.ptr % a == 0 and self.pitch % a == 0

    def get(self):
        return views.extract(self.buf.download(), self.off, self.pitch, self.n, self.rb)

    def unchanged(self, what):
        assert np.array_equal(self.buf.download(), self.before), f"{what}: an input's parent (or a refused call's output) changed"

    def written(self, start_pos, what):
        """the rows [start_pos, n) after a call that wrote them, everything around them checked"""
        views.outside_untouched(self.before, self.buf.download(), self.off, self.pitch, self.n, self.rb, start_pos, what)
        return self.get()


def launched(hip, call):
    """{family: launches} of one call"""
    hip.prof_enable(True)
    try:
        call()
        return {k: v[0] for k, v in hip.prof_read().items()}
    finally:
        hip.prof_enable(False)


def blank(rows, byte=0x5A):
    return np.full_like(rows, byte)


# ------------------------------------------------------------------------------------------------------------ row-wise

ROWWISE_SHAPES = [(256, 4, 0),      # the generic kernels (rope: four Q8 rows are the wave kernel's)
                  (256, 4, 1),      # ... three new rows: generic everywhere
                  (2048, 5, 1),     # four new 2048-wide rows: the rms / rope wave kernels and, by class, their fallbacks
                  (2048, 17, 1)]    # 16 rows: exactly rows * d = 32768, k_elementwise_q8x2 / _f16x8 and their fallbacks

# (x, out)
RMS_COMBOS = [(CONTROL, CONTROL), (C16, C16), (C8, C4), (C4, C8), (C4, C2), (C2, C16), (C2W, C34), (C34, C2W), (C16, C2W)]
ROPE_CLASSES = views.CLASSES
# silu / mul / add have ONE pitch for all operands: (pitch - row_bytes, offsets of a, b, out)
EW_COMBOS = [(0, (0, 0, 0)), (16, (16, 16, 16)), (16, (0, 32, 16)),
             (8, (8, 4, 16)), (4, (4, 4, 4)), (8, (16, 16, 16)),
             (16, (2, 16, 16)), (16, (16, 2, 16)), (16, (16, 16, 2)),       # one operand alone off the wide form's alignment
             (2, (2, 2, 2)), (14, (2, 16, 4)), (34, (34, 0, 2))]


@pytest.mark.parametrize("ad", [F16, Q8])
@pytest.mark.parametrize("d,n,sp", ROWWISE_SHAPES)
def test_rms_norm_views(hip, oracle, ad, d, n, sp):
    r = rng(d + n + sp)
    x, _ = act_rows(oracle, r, n, d, ad)
    w = (1 + 0.05 * r.standard_normal(d)).astype(np.float16)
    want = blank(x)
    oracle.rms_norm(x, ad, w, want, n, d, sp)
    wave_shape = ad == Q8 and d == 2048 and n - sp >= 4
    control = None
    # (the weights: a dense upload, and once two bytes into one -- the wave kernel reads them in 16-byte pieces)
    for xc, oc, w_off in [c + (0,) for c in RMS_COMBOS] + [(CONTROL, CONTROL, 2)]:
        what = f"rms_norm x{xc} out{oc} w+{w_off}"
        xo, oo = Operand(hip, x, xc), Operand(hip, blank(x), oc, fill=0x3C)
        wo = Operand(hip, w.view(np.uint8).reshape(1, -1), (w_off, 0))
        fam = launched(hip, lambda: hip.rms_norm(xo.view, ad, wo.view, oo.view, n, d, sp, x_pitch=xo.pitch, out_pitch=oo.pitch))
        wide = wave_shape and xo.al(4) and oo.al(4) and wo.al(16)
        assert fam == ({NARROW: 1} if wave_shape and not wide else {"rms_norm": 1}), (what, fam)
        got = oo.written(sp, what)
        xo.unchanged(what), wo.unchanged(what)
        compare_rows(got[sp:], want[sp:], ad, d, what)
        if control is None:
            control = got
            assert not wave_shape or wide, "the control takes the wave kernel"
        # one kernel for f16; the Q8 wave kernel is bit-identical to the row kernel (tests/test_ops_gpu.py)
        assert np.array_equal(got[sp:], control[sp:]), what


@pytest.mark.parametrize("ad", [F16, Q8])
@pytest.mark.parametrize("d,n,sp", ROWWISE_SHAPES)
def test_rotary_emb_views(hip, oracle, ad, d, n, sp):
    r = rng(3 * d + n + sp)
    x, _ = act_rows(oracle, r, n, d, ad)
    want = x.copy()
    oracle.rotary_emb(want, ad, n, d, 64, sp)
    wave_shape = ad == Q8 and n - sp >= 4
    control = None
    for cls in ROPE_CLASSES:
        what = f"rope {cls}"
        xo = Operand(hip, x, cls)
        fam = launched(hip, lambda: hip.rotary_emb(xo.view, ad, n, d, 64, sp, pitch=xo.pitch))
        assert fam == ({NARROW: 1} if wave_shape and not xo.al(4) else {"rotary_emb": 1}), (what, fam)
        got = xo.written(sp, what)
        compare_rows(got, want, ad, d, what, min_exact=0.999)
        control = got if control is None else control
        assert np.array_equal(got, control), what       # (wave kernel = row kernel bit for bit: tests/test_ops_gpu.py)


@pytest.mark.parametrize("ad", [F16, Q8])
@pytest.mark.parametrize("d,n,sp", ROWWISE_SHAPES)
def test_silu_mul_add_views(hip, oracle, ad, d, n, sp):
    r = rng(5 * d + n + sp)
    x, _ = act_rows(oracle, r, n, d, ad)
    y, _ = act_rows(oracle, r, n, d, ad)
    wide_shape = (n - sp) * d >= 32768
    wide_al = 4 if ad == Q8 else 16
    for name in ("silu", "mul", "add"):
        ofn, hfn = getattr(oracle, name), getattr(hip, name)
        two = name != "silu"
        want = blank(x)
        if two:
            ofn(x, y, want, ad, n, d, sp)
        else:
            ofn(x, want, ad, n, d, sp)
        control = {}
        for pad, (a_off, b_off, o_off) in EW_COMBOS:
            for inplace in (False, True):
                what = f"{name}{' in place' if inplace else ''} pad {pad} a+{a_off} b+{b_off} out+{o_off}"
                ao, bo = Operand(hip, x, (a_off, pad)), Operand(hip, y, (b_off, pad), fill=0x77)
                oo = ao if inplace else Operand(hip, blank(x), (o_off, pad), fill=0x3C)
                args = (ao.view, bo.view, oo.view) if two else (ao.view, oo.view)
                fam = launched(hip, lambda: hfn(*args, ad, n, d, sp, pitch=ao.pitch))
                used = [ao, oo] + ([bo] if two else [])
                wide = wide_shape and all(o.al(wide_al) for o in used)
                assert fam == ({NARROW: 1} if wide_shape and not wide else {"elementwise": 1}), (what, fam)
                got = oo.written(sp, what)
                bo.unchanged(what)
                if not inplace:
                    ao.unchanged(what)
                if two:
                    assert np.array_equal(got[sp:], want[sp:]), what + ": must be bit-exact"
                else:
                    compare_rows(got[sp:], want[sp:], ad, d, what, min_exact=0.995)
                # the same kernel on the same rows: the same bytes (silu across kernels is left to the oracle's band)
                first = control.setdefault(wide, got)
                assert np.array_equal(got[sp:], first[sp:]), what
        assert (True in control) == wide_shape, "the control took the wide kernel wherever the shape has one"
        assert not wide_shape or False in control, "some class left the wide kernel"


# -------------------------------------------------------------------------------------------------------------- matmul

MM_SHAPES = [(3, 256, 96, 1),        # the row kernel
             (17, 256, 96, 1),       # 16 new rows: the matrix cores
             (40, 2048, 256, 0)]     # ... and rows <= 128 with a Q8 output: the K loop is shared, k_splitk_finish rounds the rows
# (x, out)
MM_COMBOS = [(CONTROL, CONTROL), (C16, C16), (C8, C4), (C4, C8), (C2, C2), (C2W, C34), (C34, C2W), (C16, C2), (C2, C16)]
MM_COMBOS_F32 = [c for c in MM_COMBOS if c[1][0] % 4 == 0 and c[1][1] % 4 == 0] + [(C2, C4), (C2W, C8), (C34, C16)]


@pytest.mark.parametrize("name,wd,ad", MODES())
@pytest.mark.parametrize("n,d_in,d_out,sp", MM_SHAPES)
def test_matmul_2d_views(hip, oracle, name, wd, ad, n, d_in, d_out, sp):
    r = rng(n * 17 + d_in + d_out)
    x, _ = act_rows(oracle, r, n, d_in, ad)
    w, _ = weight_rows(oracle, r, d_out, d_in, wd)
    wdv = hip.upload_weight(w, wd, d_out, d_in)
    mfma_shape = n - sp >= 16
    for exact_form in ((True, False) if mfma_shape and wd != F16 else (True,)):
        hip.set_prefill_exact(exact_form)
        try:
            for od in (ad, F32):
                want = blank(np.zeros((n, row_bytes(od, d_out)), np.uint8))
                oracle.matmul_2d(x, ad, w, wd, want, od, n, d_in, d_out, sp)
                control, control_fam = {}, None
                for xc, oc in (MM_COMBOS_F32 if od == F32 else MM_COMBOS):
                    what = f"matmul {name}->{od} {'exact' if exact_form else 'fast'} x{xc} out{oc}"
                    xo, oo = Operand(hip, x, xc), Operand(hip, blank(want), oc, fill=0x3C)
                    fam = launched(hip, lambda: hip.matmul_2d(xo.view, ad, wdv, wd, oo.view, od, n, d_in, d_out, sp,
                                                              x_pitch=xo.pitch, out_pitch=oo.pitch))
                    if not mfma_shape:
                        form = "row"
                        assert fam == {"matmul_2d": 1}, (what, fam)
                    elif ad == F16:
                        # the GEMM reads the caller's f16 rows in 16-byte pieces: any other view takes the row kernel
                        form = "mfma" if xo.al(16) else "row"
                        assert fam == ({"matmul_2d_mfma": 1} if xo.al(16) else {NARROW: 1}), (what, fam)
                    else:
                        # the GEMM reads the library's f16 copy: k_act_to_f16_x2 (dwords) or k_act_to_f16 (half-words) writes it
                        form = "mfma"
                        control_fam = control_fam or fam
                        assert set(control_fam) == {"matmul_2d_mfma"} and control_fam["matmul_2d_mfma"] >= 2, control_fam
                        if xo.al(4):
                            assert fam == control_fam, (what, fam)
                        else:
                            assert fam == {NARROW: 1, "matmul_2d_mfma": control_fam["matmul_2d_mfma"] - 1}, (what, fam)
                    got = oo.written(sp, what)
                    xo.unchanged(what)
                    if form == "row" or exact_form:
                        compare_rows(got[sp:], want[sp:], od, d_out, what, atol=8e-6)
                    elif od == F32:
                        g, t = got[sp:].view(np.float32), want[sp:].view(np.float32)
                        rms = np.sqrt((t * t).mean(axis=1, keepdims=True))
                        assert (np.abs(g - t) <= 2e-3 * rms + 1e-7).all(), (what, float((np.abs(g - t) / rms).max()))
                    else:
                        compare_rows(got[sp:], want[sp:], od, d_out, what, min_exact=0.80, steps=2.0, atol=2e-4)
                    # the same kernels on the same rows (either conversion writes the same f16 copy): the same bytes
                    first = control.setdefault(form, got)
                    assert np.array_equal(got[sp:], first[sp:]), what
                if mfma_shape:
                    assert "mfma" in control
                    assert ad != F16 or "row" in control, "some class left the matrix-core kernel"
        finally:
            hip.set_prefill_exact(False)
    if mfma_shape and (n, d_in, d_out) == (40, 2048, 256) and wd != F16:
        # (the fast form's Q8 output above took three launches: conversion, GEMM over a shared K loop, k_splitk_finish)
        xo, oo = Operand(hip, x, CONTROL), Operand(hip, np.zeros((n, row_bytes(Q8, d_out)), np.uint8), C2)
        fam = launched(hip, lambda: hip.matmul_2d(xo.view, ad, wdv, wd, oo.view, Q8, n, d_in, d_out, sp, out_pitch=oo.pitch))
        assert fam == {"matmul_2d_mfma": 3}, fam


@pytest.mark.parametrize("name,wd,ad", MODES())
def test_token_embed_views(hip, oracle, name, wd, ad):
    r = rng(5)
    V, d, sp = 50, 256, 1
    w, _ = weight_rows(oracle, r, V, d, wd)
    wdv = hip.upload_weight(w, wd, V, d)
    toks = np.array([3, 49, 0, 7, 7], np.int32)
    n = len(toks)
    want = blank(np.zeros((n, row_bytes(ad, d)), np.uint8))
    oracle.token_embed(w, wd, toks, want, ad, d, sp)
    for cls, t_off in [(c, 0) for c in views.CLASSES] + [(C2W, 4)]:
        what = f"token_embed {name} out{cls} tokens+{t_off}"
        oo = Operand(hip, blank(want), cls, fill=0x3C)
        to = Operand(hip, toks.view(np.uint8).reshape(1, -1), (t_off, 0))
        fam = launched(hip, lambda: hip.token_embed(wdv, wd, V, to.view, oo.view, ad, n, d, sp, out_pitch=oo.pitch))
        assert fam == {"token_embed": 1}, (what, fam)
        got = oo.written(sp, what)
        to.unchanged(what)
        assert np.array_equal(got[sp:], want[sp:]), what + ": a copy / exact requantisation, must be bit-exact"


# ----------------------------------------------------------------------------------------------------------- attention

# (q, k, v, out); k and v share one pitch: v's class keeps its offset and takes k's padding
ATTN_COMBOS = [(CONTROL, CONTROL, CONTROL, CONTROL), (C16, C16, C16, C16), (C2, C2, C2, C2),
               (C8, C4, C16, C2W), (C34, C2W, C2, C8), (C4, C34, C16, C16),
               (C16, C16, C16, C2), (C16, C16, C8, C16), (C16, C8, C16, C16), (C8, C16, C16, C16), (C16, C16, C16, C4)]


@pytest.mark.parametrize("ad", [F16, Q8])
@pytest.mark.parametrize("n,sp", [(5, 0), (40, 3)])
def test_qkv_attn_views(hip, oracle, ad, n, sp):
    H, G, dh = 4, 2, 64
    r = rng(n * 7 + sp)
    q, _ = act_rows(oracle, r, n, H * dh, ad)
    k, _ = act_rows(oracle, r, n, G * dh, ad)
    v, _ = act_rows(oracle, r, n, G * dh, ad)
    want = blank(q)
    oracle.qkv_attn(q, k, v, want, ad, n, H, G, dh, sp)
    tiled_shape = n - sp >= 16
    for exact_form in ((True, False) if tiled_shape and ad == Q8 else (False,)):
        hip.set_prefill_exact(exact_form)
        try:
            control = {}
            for qc, kc, vc, oc in ATTN_COMBOS:
                what = f"qkv_attn {'exact' if exact_form else 'fast'} q{qc} k{kc} v{vc} out{oc}"
                qo, ko, vo = Operand(hip, q, qc), Operand(hip, k, kc, fill=0x77), Operand(hip, v, (vc[0], kc[1]), fill=0x19)
                oo = Operand(hip, blank(q), oc, fill=0x3C)
                fam = launched(hip, lambda: hip.qkv_attn(qo.view, ko.view, vo.view, oo.view, ad, n, H, G, dh, sp,
                                                         q_pitch=qo.pitch, kv_pitch=ko.pitch, out_pitch=oo.pitch))
                if not tiled_shape:
                    form = "row"
                    assert fam == {"qkv_attn": 1}, (what, fam)
                elif ad == Q8:
                    form = "tiled"                                   # written for 2-byte alignment: every view stays
                    assert fam == {"qkv_attn_tiled": 1}, (what, fam)
                else:
                    wide = qo.al(16) and ko.al(16) and vo.al(16) and oo.al(4)
                    form = "tiled" if wide else "row"
                    assert fam == ({"qkv_attn_tiled": 1} if wide else {NARROW: 1}), (what, fam)
                got = oo.written(sp, what)
                qo.unchanged(what), ko.unchanged(what), vo.unchanged(what)
                compare_rows(got[sp:], want[sp:], ad, H * dh, what, min_exact=0.90, steps=2.0,
                             atol=2e-3 if ad == F16 and form == "tiled" else 2e-4)
                first = control.setdefault(form, got)
                assert np.array_equal(got[sp:], first[sp:]), what      # (the same kernel on the same rows)
            if tiled_shape:
                assert "tiled" in control
                assert ad != F16 or "row" in control, "some class left the tiled f16 kernel"
        finally:
            hip.set_prefill_exact(False)


# --------------------------------------------------------------------------------------------------------- copy_ranges

COPY_SIZES = [0, 1, 3, 4, 68, 4080, 4112]
COPY_SLOT = 4352                      # 17 * 256: a range's slot -- 64 bytes of guard, up to 63 of misalignment, the bytes, guard
# (source, destination) offsets inside 64 bytes: the kernel copies a range in 16-byte pieces when both addresses and the
# size are multiples of 16, in dwords when they are multiples of 4, in bytes otherwise
COPY_ALIGN = [(0, 0), (16, 48), (0, 8), (4, 12), (16, 4), (1, 0), (2, 2), (3, 17), (16, 1)]


def _copy_case(hip, cases):
    """cases: [(bytes, src offset, dst offset)], one slot each -> (ranges, src buffer, dst buffer, src bytes, dst before, dst expected)"""
    total = COPY_SLOT * len(cases)
    src = rng(len(cases)).integers(0, 256, total, dtype=np.uint8)
    before = views.canaries(total, 0x42)
    sb, db = hip.upload(src), hip.upload(before)
    assert sb.ptr % 256 == 0 and db.ptr % 256 == 0
    want = before.copy()
    ranges = []
    for i, (nb, so, do) in enumerate(cases):
        s0, d0 = i * COPY_SLOT + 64 + so, i * COPY_SLOT + 64 + do
        assert d0 + nb + 64 <= (i + 1) * COPY_SLOT
        want[d0:d0 + nb] = src[s0:s0 + nb]
        ranges.append((db.ptr + d0, sb.ptr + s0, nb))
    return ranges, sb, db, src, before, want


def test_copy_ranges_every_tier_against_numpy(hip):
    cases = [(nb, so, do) for nb in COPY_SIZES for so, do in COPY_ALIGN]
    assert len(cases) <= 64
    tiers = {16 if (nb | so | do) % 16 == 0 else 4 if (nb | so | do) % 4 == 0 else 1 for nb, so, do in cases if nb}
    assert tiers == {16, 4, 1}, "every tier of k_copy_ranges is reached"
    for nb in (68, 4080, 4112):
        assert {(nb | so | do) % 4 == 0 for so, do in COPY_ALIGN} == {True, False}
    ranges, sb, db, src, before, want = _copy_case(hip, cases)
    fam = launched(hip, lambda: hip.copy_ranges(ranges))
    assert fam == {"elementwise": 1}, fam
    got = db.download()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{bad.size} bytes differ from numpy's copies (guards included); the first in slot {int(bad[0]) // COPY_SLOT}",
                           cases[int(bad[0]) // COPY_SLOT], int(bad[0]) % COPY_SLOT)
    assert np.array_equal(sb.download(), src)


def test_copy_ranges_the_most_ranges_and_refusals(hip):
    from __graft_entry__ import load_package
    pkg = load_package()
    cases = [(COPY_SIZES[i % 7], COPY_ALIGN[i % 9][0], COPY_ALIGN[(i // 7) % 9][1]) for i in range(64)]
    ranges, sb, db, src, before, want = _copy_case(hip, cases)
    hip.copy_ranges(ranges)
    assert np.array_equal(db.download(), want)
    assert np.array_equal(sb.download(), src)
    # 65 ranges, and a range without a destination / a source: refused, nothing copied
    db.upload(before)
    for bad in (ranges + ranges[:1], ranges[:3] + [(0, ranges[3][1], 4)], [(ranges[0][0], 0, 4)] + ranges[1:5]):
        fam = launched(hip, lambda: hip.copy_ranges_rc(bad))
        assert fam == {}, fam
        assert hip.copy_ranges_rc(bad) != 0
        assert "copy_ranges" in hip.last_error()
        assert np.array_equal(db.download(), before)
    with pytest.raises(pkg.GtenHipError, match="copy_ranges"):
        hip.copy_ranges(ranges + ranges[:1])
    assert hip.copy_ranges_rc([]) == 0


# ------------------------------------------------------------------------------------------------------------ refusals

ODD = [((1, 0), "an odd base"), ((0, 1), "an odd pitch"), ((1, 1), "both odd")]


def _refused(hip, op, call, operands, what):
    """the call returns non-zero, the message names the operator, nothing ran, no parent changed"""
    got = {}

    def run():
        got["rc"] = call()
    fam = launched(hip, run)
    assert got["rc"] != 0, what + ": accepted"
    assert op in hip.last_error(), (what, hip.last_error())
    assert fam == {}, (what, fam)
    for o in operands:
        o.unchanged(what)


@pytest.mark.parametrize("ad", [F16, Q8])
def test_rowwise_ops_refuse_odd_views(hip, oracle, ad):
    r = rng(41)
    n, d = 4, 256
    x, _ = act_rows(oracle, r, n, d, ad)
    w = hip.upload(np.ones(d, np.float16))
    for slot in range(3):                                            # which operand is off: a, b / out
        for cls, why in ODD:
            cl = [CONTROL] * 3
            cl[slot] = cls
            pad = cls[1]
            # rms_norm: x and out with pitches of their own
            if slot < 2:
                xo, oo = Operand(hip, x, cl[0]), Operand(hip, blank(x), cl[1])
                _refused(hip, "rms_norm", lambda: hip.rms_norm_rc(xo.view, ad, w, oo.view, n, d, 0, x_pitch=xo.pitch, out_pitch=oo.pitch),
                         [xo, oo], f"rms_norm, {why} of operand {slot}")
            if slot == 0:
                xo = Operand(hip, x, cls)
                _refused(hip, "rotary_emb", lambda: hip.rotary_emb_rc(xo.view, ad, n, d, 64, 0, pitch=xo.pitch), [xo], f"rotary_emb, {why}")
                wo = Operand(hip, np.ones((1, 2 * d), np.uint8), (1, 0))
                xo, oo = Operand(hip, x, CONTROL), Operand(hip, blank(x), CONTROL)
                _refused(hip, "rms_norm", lambda: hip.rms_norm_rc(xo.view, ad, wo.view, oo.view, n, d, 0), [xo, oo], "rms_norm, odd weights")
            # silu / mul / add: one pitch; an odd pitch is everybody's, an odd base one operand's
            ops = [Operand(hip, x, (c[0], pad)) for c in cl]
            a, b, o = ops
            if slot != 1:
                _refused(hip, "silu", lambda: hip.silu_rc(a.view, o.view, ad, n, d, 0, pitch=a.pitch), ops, f"silu, {why} of operand {slot}")
            _refused(hip, "mul", lambda: hip.mul_rc(a.view, b.view, o.view, ad, n, d, 0, pitch=a.pitch), ops, f"mul, {why} of operand {slot}")
            _refused(hip, "add", lambda: hip.add_rc(a.view, b.view, o.view, ad, n, d, 0, pitch=a.pitch), ops, f"add, {why} of operand {slot}")
    from __graft_entry__ import load_package
    xo = Operand(hip, x, (1, 1))
    with pytest.raises(load_package().GtenHipError, match="silu"):
        hip.silu(xo.view, xo.view, ad, n, d, 0, pitch=xo.pitch)


@pytest.mark.parametrize("name,wd,ad", MODES())
def test_matmul_2d_and_token_embed_refuse_views_outside_the_contract(hip, oracle, name, wd, ad):
    r = rng(43)
    d_in, d_out, V = 256, 96, 50
    w, _ = weight_rows(oracle, r, d_out, d_in, wd)
    wdv = hip.upload_weight(w, wd, d_out, d_in)
    for n in (3, 17):                                                # the row kernel's shape and the matrix cores'
        x, _ = act_rows(oracle, r, n, d_in, ad)
        for od in (ad, F32):
            out = np.zeros((n, row_bytes(od, d_out)), np.uint8)
            bad = ODD + ([((2, 0), "a base that is no multiple of 4"), ((0, 2), "a pitch that is no multiple of 4"),
                          ((6, 4), "a base that is no multiple of 4"), ((4, 6), "a pitch that is no multiple of 4")] if od == F32 else [])
            for cls, why in bad:
                xo, oo = Operand(hip, x, CONTROL), Operand(hip, out, cls)
                _refused(hip, "matmul_2d", lambda: hip.matmul_2d_rc(xo.view, ad, wdv, wd, oo.view, od, n, d_in, d_out, 0, out_pitch=oo.pitch),
                         [xo, oo], f"matmul {name}->{od} n={n}: {why} of the output")
            for cls, why in ODD:
                xo, oo = Operand(hip, x, cls), Operand(hip, out, CONTROL)
                _refused(hip, "matmul_2d", lambda: hip.matmul_2d_rc(xo.view, ad, wdv, wd, oo.view, od, n, d_in, d_out, 0, x_pitch=xo.pitch),
                         [xo, oo], f"matmul {name}->{od} n={n}: {why} of the input")
        wo = Operand(hip, np.zeros((1, 64), np.uint8), (8, 0))
        xo, oo = Operand(hip, x, CONTROL), Operand(hip, np.zeros((n, row_bytes(ad, d_out)), np.uint8), CONTROL)
        _refused(hip, "matmul_2d", lambda: hip.matmul_2d_rc(xo.view, ad, wo.view, wd, oo.view, ad, n, d_in, d_out, 0), [xo, oo],
                 "matmul: weights 8 bytes into an allocation")
    ew, _ = weight_rows(oracle, r, V, d_in, wd)
    ewd = hip.upload_weight(ew, wd, V, d_in)
    toks = np.array([1, 2, 3], np.int32)
    out = np.zeros((3, row_bytes(ad, d_in)), np.uint8)
    for cls, why in ODD:
        to, oo = Operand(hip, toks.view(np.uint8).reshape(1, -1), CONTROL), Operand(hip, out, cls)
        _refused(hip, "token_embed", lambda: hip.token_embed_rc(ewd, wd, V, to.view, oo.view, ad, 3, d_in, 0, out_pitch=oo.pitch), [to, oo],
                 f"token_embed {name}: {why} of the output")
    for t_off in (1, 2):
        to, oo = Operand(hip, toks.view(np.uint8).reshape(1, -1), (t_off, 0)), Operand(hip, out, CONTROL)
        _refused(hip, "token_embed", lambda: hip.token_embed_rc(ewd, wd, V, to.view, oo.view, ad, 3, d_in, 0), [to, oo],
                 f"token_embed {name}: tokens {t_off} bytes off")


@pytest.mark.parametrize("ad", [F16, Q8])
@pytest.mark.parametrize("n", [5, 40])
def test_qkv_attn_refuses_odd_views(hip, oracle, ad, n):
    H, G, dh = 4, 2, 64
    r = rng(47)
    q, _ = act_rows(oracle, r, n, H * dh, ad)
    k, _ = act_rows(oracle, r, n, G * dh, ad)
    for slot, who in enumerate(("q", "k", "v", "out")):
        for cls, why in ODD:
            cl = [CONTROL] * 4
            cl[slot] = cls
            kv_pad = cls[1] if slot in (1, 2) else 0                 # (k and v share their pitch)
            qo, oo = Operand(hip, q, cl[0]), Operand(hip, blank(q), cl[3])
            ko, vo = Operand(hip, k, (cl[1][0], kv_pad)), Operand(hip, k, (cl[2][0], kv_pad))
            _refused(hip, "qkv_attn", lambda: hip.qkv_attn_rc(qo.view, ko.view, vo.view, oo.view, ad, n, H, G, dh, 0, q_pitch=qo.pitch,
                                                             kv_pitch=ko.pitch, out_pitch=oo.pitch), [qo, ko, vo, oo], f"qkv_attn n={n}: {why} of {who}")
