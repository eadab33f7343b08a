"""-m gpu: prompt rows behind PER-SEGMENT contexts (include/gten_hip_continue.h).  One row matrix holds the new
rows of several conversations; segment s continues its own K / V rows [0, len_s).  Every comparison is byte EQUALITY on
the same build: against the whole prompts as segments of gten_hip_block_rows, and against gten_hip_block_rows_prefixed."""
import numpy as np
import pytest

from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from helpers import F16, Q4, Q8, act_rows, rng, row_bytes
from test_block_rows_gpu import alloc_acts, make_block

pytestmark = pytest.mark.gpu

E, H, KVH, F = 256, 4, 2, 512                     # the block of tests/test_prefix_gpu.py
# the 3.9 boundaries between the two K / V sources, mixed in ONE launch: the smallest context (16), inside a 16-lane column
# group (40), at a 256-position tile edge (256), inside a 64-position V sub-tile of the second tile (270)
CONTEXTS = (16, 40, 256, 270)
ROWS = (16, 17, 33, 50)                           # 17 and 33: partial row tiles
COMPARED = ("k", "v", "attn_out", "h", "out")

_blocks = {}
_runs = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_buffers():
    yield
    _blocks.clear()
    _runs.clear()


def block_of(hip, oracle, wd):
    if wd not in _blocks:
        _blocks[wd] = make_block(hip, oracle, rng(1700 + wd), wd, E, H, KVH, F, 0)
    return _blocks[wd]


def ints_of(wd):
    return dict(adtype=F16 if wd == F16 else Q8, wdtype=wd, n_embd=E, n_heads=H, n_kv_heads=KVH, n_ffn=F)


def starts_of(lens):
    out = [0]
    for n in lens:
        out.append(out[-1] + n)
    return out


def rows_of(buf, n, rb):
    return buf.download(nbytes=n * rb).reshape(n, rb).copy()


def run_of(hip, oracle, wd, exact):
    """The reference of the module, computed once per (weights, form) and left unchanged: the whole prompts (context + rows) as
    segments of block_rows, each prompt's context K / V rows in a buffer of its own, and the ONE continued call over the
    four segments.  Returns numpy rows per compared buffer and the device buffers of the contexts."""
    key = (wd, exact)
    if key in _runs:
        return _runs[key]
    ad = F16 if wd == F16 else Q8
    w, widths = block_of(hip, oracle, wd)
    r = rng(1800 + wd)
    ctx_rows = [act_rows(oracle, r, n, E, ad)[0] for n in CONTEXTS]
    new_rows = [act_rows(oracle, r, n, E, ad)[0] for n in ROWS]
    w_starts = starts_of([c + n for c, n in zip(CONTEXTS, ROWS)])
    s_starts = starts_of(ROWS)
    n_whole, n_new = w_starts[-1], s_starts[-1]
    ints = ints_of(wd)
    hip.set_prefill_exact(exact)
    try:
        a_whole = alloc_acts(hip, widths, n_whole, 0, ad)
        bufs = dict(w)
        bufs.update(a_whole)
        bufs["inp"] = hip.upload(np.concatenate([np.concatenate([c, n]) for c, n in zip(ctx_rows, new_rows)]))
        hip.set_row_segments(w_starts)
        assert hip.block_rows(n_whole, 0, ints, bufs)
        hip.sync()
        whole = {name: rows_of(a_whole[name], n_whole, row_bytes(ad, widths[name])) for name in COMPARED}
        # each prompt's context: its own whole-prompt K / V rows, in buffers of their own (16-byte aligned)
        kv = [(hip.upload(whole["k"][w_starts[s]:w_starts[s] + c]), hip.upload(whole["v"][w_starts[s]:w_starts[s] + c])) for s, c in enumerate(CONTEXTS)]
        a_got = alloc_acts(hip, widths, n_new, 0x5a, ad)
        bufs = dict(w)
        bufs.update(a_got)
        bufs["inp"] = hip.upload(np.concatenate(new_rows))
        hip.set_row_segments(s_starts)
        hip.set_row_contexts([[(k, v, c) for (k, v), c in zip(kv, CONTEXTS)]])
        assert hip.block_rows_continued(n_new, ints, bufs, 0)
        hip.sync()
        got = {name: rows_of(a_got[name], n_new, row_bytes(ad, widths[name])) for name in COMPARED}
    finally:
        hip.set_row_contexts(None)
        hip.set_row_segments(None)
        hip.set_prefill_exact(False)
    _runs[key] = dict(whole=whole, got=got, kv=kv, new_rows=new_rows, w_starts=w_starts, s_starts=s_starts)
    return _runs[key]


def differing(got, want):
    return np.nonzero((got != want).any(axis=1))[0]


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("wd", [Q4, Q8, F16])
def test_continued_rows_leave_the_whole_prompts_bytes(hip, oracle, wd, exact):
    run = run_of(hip, oracle, wd, exact)
    for name in COMPARED:
        want = np.concatenate([run["whole"][name][s + c:s + c + n] for s, c, n in zip(run["w_starts"], CONTEXTS, ROWS)])
        bad = differing(run["got"][name], want)
        assert bad.size == 0, (name, wd, exact, "rows that differ", bad[:8].tolist(), int(bad.size))


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("wd", [Q4, Q8, F16])
def test_each_segment_equals_the_prefixed_call_for_it_alone(hip, oracle, wd, exact):
    run = run_of(hip, oracle, wd, exact)
    ad = F16 if wd == F16 else Q8
    w, widths = block_of(hip, oracle, wd)
    hip.set_prefill_exact(exact)
    try:
        for s, (c, n) in enumerate(zip(CONTEXTS, ROWS)):
            a = alloc_acts(hip, widths, n, 0xa5, ad)
            bufs = dict(w)
            bufs.update(a)
            bufs["inp"] = hip.upload(run["new_rows"][s])
            hip.set_row_segments([0, n])
            assert hip.block_rows_prefixed(n, ints_of(wd), bufs, run["kv"][s][0], run["kv"][s][1], c)
            hip.sync()
            r0 = run["s_starts"][s]
            for name in COMPARED:
                want = rows_of(a[name], n, row_bytes(ad, widths[name]))
                bad = differing(run["got"][name][r0:r0 + n], want)
                assert bad.size == 0, (name, wd, exact, "segment", s, bad[:8].tolist())
    finally:
        hip.set_row_segments(None)
        hip.set_prefill_exact(False)


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("wd", [Q4, Q8, F16])
def test_every_context_on_one_prefix_equals_the_prefixed_call(hip, oracle, wd, exact):
    ad = F16 if wd == F16 else Q8
    w, widths = block_of(hip, oracle, wd)
    P = 40
    r = rng(1900 + wd)
    pre = {name: hip.upload(act_rows(oracle, r, P, KVH * (E // H), ad)[0]) for name in ("k", "v")}
    inp = hip.upload(np.concatenate([act_rows(oracle, r, n, E, ad)[0] for n in ROWS]))
    starts = starts_of(ROWS)
    n_new = starts[-1]
    hip.set_prefill_exact(exact)
    try:
        hip.set_row_segments(starts)
        res = []
        for continued in (False, True):
            a = alloc_acts(hip, widths, n_new, 0x33 if continued else 0x77, ad)
            bufs = dict(w)
            bufs.update(a)
            bufs["inp"] = inp
            if continued:
                # two layers of records, the second one used: the call offsets into [n_layers][n_segments]
                other = alloc_acts(hip, dict(k=widths["k"], v=widths["v"]), P, 0, ad)
                hip.set_row_contexts([[(other["k"], other["v"], P)] * len(ROWS), [(pre["k"], pre["v"], P)] * len(ROWS)])
                assert hip.block_rows_continued(n_new, ints_of(wd), bufs, 1)
            else:
                assert hip.block_rows_prefixed(n_new, ints_of(wd), bufs, pre["k"], pre["v"], P)
            hip.sync()
            res.append({name: rows_of(a[name], n_new, row_bytes(ad, widths[name])) for name in COMPARED})
        for name in COMPARED:
            bad = differing(res[1][name], res[0][name])
            assert bad.size == 0, (name, wd, exact, bad[:8].tolist())
    finally:
        hip.set_row_contexts(None)
        hip.set_row_segments(None)
        hip.set_prefill_exact(False)


def test_continued_block_rows_refusals(hip, oracle):
    pkg = load_package()
    w, widths = block_of(hip, oracle, Q8)
    a = alloc_acts(hip, widths, 64, 0, Q8)
    ctx = alloc_acts(hip, dict(k=widths["k"], v=widths["v"]), 2048, 0, Q8)
    bufs = dict(w)
    bufs.update(a)
    bufs["inp"] = hip.upload(act_rows(oracle, rng(5), 64, E, Q8)[0])
    ints = ints_of(Q8)
    k, v = ctx["k"], ctx["v"]

    def attempt(contexts, layer=0):
        hip.set_row_contexts(contexts)
        return hip.block_rows_continued(64, ints, bufs, layer)

    hip.set_row_segments(None)
    hip.set_row_contexts(None)
    try:
        with pytest.raises(pkg.GtenHipError):                  # no segments set
            attempt([[(k, v, 32), (k, v, 32)]])
        hip.set_row_segments([0, 24, 64])
        with pytest.raises(pkg.GtenHipError):                  # segments, but no contexts
            hip.block_rows_continued(64, ints, bufs, 0)
        with pytest.raises(pkg.GtenHipError):                  # three contexts for two segments
            attempt([[(k, v, 32)] * 3])
        with pytest.raises(pkg.GtenHipError):                  # one context for two segments
            attempt([[(k, v, 32)]])
        with pytest.raises(pkg.GtenHipError):                  # len 0
            attempt([[(k, v, 32), (k, v, 0)]])
        with pytest.raises(pkg.GtenHipError):                  # 2009 + 40 = 2049 positions
            attempt([[(k, v, 32), (k, v, 2009)]])
        with pytest.raises(pkg.GtenHipError):                  # an unaligned pointer
            attempt([[(k, v, 32), (k.ptr + 8, v, 32)]])
        with pytest.raises(pkg.GtenHipError):                  # a segment's len differs between layers
            attempt([[(k, v, 32), (k, v, 32)], [(k, v, 32), (k, v, 33)]])
        with pytest.raises(pkg.GtenHipError):                  # a layer the contexts were not set for
            attempt([[(k, v, 32), (k, v, 32)]], layer=1)
        hip.set_row_contexts([[(k, v, 32), (k, v, 32)]])
        hip.set_row_segments([0, 32, 64])                      # other segments: the contexts no longer apply
        with pytest.raises(pkg.GtenHipError):
            hip.block_rows_continued(64, ints, bufs, 0)
        hip.set_row_segments([0, 24, 64])
        hip.set_row_contexts([[(k, v, 32), (k, v, 32)]])
        assert not hip.block_rows_continued(64, dict(ints, n_heads=8), bufs, 0)       # not handled, as block_rows
        assert attempt([[(k, v, 2024), (k, v, 2008)]])                                 # 2024 + 24 and 2008 + 40 = 2048: taken
        hip.sync()
    finally:
        hip.set_row_contexts(None)
        hip.set_row_segments(None)
