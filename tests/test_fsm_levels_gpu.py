"""-m gpu: the automaton's rung among the sampler's levels on one decoder, in the manner of
tests/test_penalty_levels_gpu.py.  One decoder meets tables, records, cuts, the penalty and the automaton with the automaton first, in
the middle and last, then switches them off again in the same order; after every change all its graph kinds -- captured single steps,
eager steps, four-step replays -- must give what a fresh decoder with the same requests gives eagerly: ids, record bits, logits bits.

A table and an automaton do not compose on one sequence, so the automaton is bound to the odd sequences (the table is on the even ones);
a single sequence has every feature but the table."""
import numpy as np
import pytest

import fsm_ref as ref
from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from test_bias_gpu import Dec, P
from test_fsm_gpu import dec_bind
from test_penalty_gpu import dec_pen
from test_penalty_levels_gpu import PEN, pen_applies
from test_sampler_levels_gpu import FEATURES, reference, run_stage, same, sample_all, setup, switch

pytestmark = pytest.mark.gpu

OTHERS = FEATURES + ("penalty",)
ORDERS = [OTHERS[:i] + ("fsm",) + OTHERS[i:] for i in (0, 2, 4)]             # first, in the middle, last
_REF, _POOL = {}, {}


def pool(host, V):
    """sixteen live states, a quarter of the ids each: nobody ends, every step is masked"""
    if V not in _POOL:
        f = load_package().hostabi.Fsm(host, V)
        f.add_table(*ref.random_pool(np.random.default_rng(31), 16, V, 0.25, 0))
        _POOL[V] = f
    return _POOL[V]


def fsm_applies(q, n_seq):
    return n_seq == 1 or q % 2 == 1


def switch_any(d, feat, on, banned):
    if feat == "table" and d.n == 1:
        return                                                                # (the single sequence is bound to the automaton instead)
    if feat == "penalty":
        for q in range(d.n):
            if pen_applies(q, d.n):
                dec_pen(d, q, *(PEN if on else (1.0, 0.0, 0.0)))
    elif feat == "fsm":
        for q in range(d.n):
            if fsm_applies(q, d.n):
                dec_bind(d, q, (5 * q + 2) % 16 if on else -1, P + 1)
    else:
        switch(d, feat, on, banned)


def reference_fsm(n_seq, feats):
    """a fresh decoder that has the requests before its first step and runs every step eagerly"""
    if n_seq == 1:
        feats = frozenset(feats - {"table"})
    if not feats & {"penalty", "fsm"}:
        return reference(n_seq, frozenset(feats))
    if (n_seq, feats) not in _REF:
        s = setup(n_seq)
        d = Dec(s["host"], s["cfg"], s["weights"], n_seq)
        d.o.set_fsm(pool(s["host"], s["cfg"].n_vocab))
        sample_all(d)
        for f in OTHERS + ("fsm",):
            if f in feats:
                switch_any(d, f, True, s["banned"])
        _REF[(n_seq, feats)] = run_stage(d, s, "records" in feats, eager=True)
        d.o.close()
    return _REF[(n_seq, feats)]


@pytest.mark.parametrize("order", ORDERS, ids="-".join)
@pytest.mark.parametrize("n_seq", [1, 2, 16])
def test_the_automaton_first_in_the_middle_and_last(hip, n_seq, order):
    s = setup(n_seq)
    d = Dec(s["host"], s["cfg"], s["weights"], n_seq)
    d.o.set_fsm(pool(s["host"], s["cfg"].n_vocab))
    sample_all(d)
    sampling_only = run_stage(d, s, False)
    same(sampling_only, reference(n_seq, frozenset()), "sampling")           # a pool alone changes nothing
    assert not d.o.fsm_info()[3]
    assert reference_fsm(n_seq, frozenset(["fsm"]))[0].tolist() != sampling_only[0].tolist()          # (the automaton moves ids)
    active = set()
    for on in (True, False):
        for feat in order:
            switch_any(d, feat, on, s["banned"])
            active ^= {feat}
            got = run_stage(d, s, "records" in active)
            same(got, reference_fsm(n_seq, frozenset(active)), (feat, on, sorted(active)))
            assert d.o.fsm_info()[3] == (on is False or "fsm" in active)      # the rung stays once taken
    assert not active and got[0].tolist() == sampling_only[0].tolist()
    assert d.sampler_launches() == 1 and (d.o.fsm_info()[1] == -1).all()
    # a greedy decoder with a binding alone ends its step in the sampler launch, and in the argmax again once it is unbound
    for q in range(n_seq):
        d.request(q, 0)
    assert d.sampler_launches() == 0
    q1 = 0 if n_seq == 1 else 1
    dec_bind(d, q1, 3, P + 1)
    assert d.sampler_launches() == 1
    dec_bind(d, q1, -1)
    assert d.sampler_launches() == 0
    same(run_stage(d, s, False), reference(n_seq, None), "nothing set, at the end")
    d.o.close()
