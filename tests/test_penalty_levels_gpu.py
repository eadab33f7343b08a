"""-m gpu: the penalty's rung among the sampler's levels on one decoder, in the manner of
tests/test_sampler_levels_gpu.py.  One decoder meets tables, records, cuts and the penalty with the penalty first, second, third and
last, then switches them off again in the same order; after every change all its graph kinds -- captured single steps, eager steps,
four-step replays -- must give what a fresh decoder with the same requests gives eagerly: ids, record bits, logits bits."""
import numpy as np
import pytest

from gpu_common import hip  # noqa: F401
from test_bias_gpu import Dec
from test_penalty_gpu import dec_pen, dec_pen_info
from test_sampler_levels_gpu import FEATURES, applies, reference, run_stage, same, sample_all, setup, switch

pytestmark = pytest.mark.gpu

PEN = (1.3, 0.4, 0.2, 2, 9)              # (r, freq, pres, start, last_n): a window that starts inside the prompt and is shorter than the run
ORDERS = [FEATURES[:i] + ("penalty",) + FEATURES[i:] for i in range(4)]
_REF = {}


def pen_applies(q, n_seq):
    """the penalty on two sequences of three (a single sequence has it)"""
    return n_seq == 1 or q % 3 != 1


def switch_any(d, feat, on, banned):
    if feat != "penalty":
        return switch(d, feat, on, banned)
    for q in range(d.n):
        if pen_applies(q, d.n):
            dec_pen(d, q, *(PEN if on else (1.0, 0.0, 0.0)))


def reference_pen(n_seq, feats):
    """tests/test_sampler_levels_gpu.py's reference, with the penalty among the features of the fresh eager decoder"""
    if "penalty" not in feats:
        return reference(n_seq, frozenset(feats))
    if (n_seq, feats) not in _REF:
        s = setup(n_seq)
        d = Dec(s["host"], s["cfg"], s["weights"], n_seq)
        sample_all(d)
        for f in FEATURES + ("penalty",):
            if f in feats:
                switch_any(d, f, True, s["banned"])
        _REF[(n_seq, feats)] = run_stage(d, s, "records" in feats, eager=True)
        d.o.close()
    return _REF[(n_seq, feats)]


@pytest.mark.parametrize("order", ORDERS, ids="-".join)
@pytest.mark.parametrize("n_seq", [1, 2, 16])
def test_the_penalty_first_second_third_and_last(hip, n_seq, order):
    s = setup(n_seq)
    d = Dec(s["host"], s["cfg"], s["weights"], n_seq)
    sample_all(d)
    sampling_only = run_stage(d, s, False)
    same(sampling_only, reference(n_seq, frozenset()), "sampling")
    assert reference_pen(n_seq, frozenset(["penalty"]))[0].tolist() != sampling_only[0].tolist()       # (the penalty moves ids)
    active = set()
    for on in (True, False):
        for feat in order:
            switch_any(d, feat, on, s["banned"])
            active ^= {feat}
            got = run_stage(d, s, "records" in active)
            same(got, reference_pen(n_seq, frozenset(active)), (feat, on, sorted(active)))
            assert dec_pen_info(d)[5] == (on is False or "penalty" in active)                         # the rung stays once taken
    assert not active and got[0].tolist() == sampling_only[0].tolist()
    assert d.sampler_launches() == 1
    r, f, p, st, ln, ever = dec_pen_info(d)
    assert ever and (r == 1.0).all() and not f.any() and not p.any() and not st.any() and not ln.any()
    # a greedy decoder with a penalty alone ends its step in the sampler launch, and in the argmax again once it is cleared
    for q in range(n_seq):
        d.request(q, 0)
    assert d.sampler_launches() == 0
    dec_pen(d, 0, *PEN)
    assert d.sampler_launches() == 1
    dec_pen(d, 0, 1.0, 0.0, 0.0)
    assert d.sampler_launches() == 0
    same(run_stage(d, s, False), reference(n_seq, None), "nothing set, at the end")
    d.o.close()
