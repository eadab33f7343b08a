"""-m gpu: Mirostat's rung among the sampler's levels on one decoder, in the manner of
tests/test_fsm_levels_gpu.py.  One decoder meets tables, records, cuts, the penalty, the automaton and Mirostat with Mirostat first, in
the middle and last, then switches them off again in the same order; after every change all its graph kinds -- captured single steps,
eager steps, four-step replays -- must give what a fresh decoder with the same requests gives eagerly: ids, record bits, logits bits.

A cut and Mirostat do not compose on one sequence, so Mirostat is bound to the even sequences (the cut is on the odd ones, the table on the
even ones: Mirostat under a table); a single sequence has every feature but the table (it is bound to the automaton) and the cut."""
import pytest

from gpu_common import hip  # noqa: F401
from test_bias_gpu import Dec, P
from test_fsm_levels_gpu import OTHERS as FIVE_BUT_FSM
from test_fsm_levels_gpu import pool, reference_fsm
from test_fsm_levels_gpu import switch_any as switch_five
from test_mirostat_decoder_gpu import dec_miro
from test_sampler_levels_gpu import reference, run_stage, same, sample_all, setup

pytestmark = pytest.mark.gpu

OTHERS = FIVE_BUT_FSM + ("fsm",)                                              # table, records, cut, penalty, fsm
ORDERS = [OTHERS[:i] + ("miro",) + OTHERS[i:] for i in (0, 2, 5)]             # first, in the middle, last
MIRO = (3.0, 0.25, 2 << 16)                                                   # tau, eta, mu at the first decoded position
_REF = {}


def miro_applies(q, n_seq):
    return n_seq == 1 or q % 2 == 0


def switch_any(d, feat, on, banned):
    if feat == "cut" and d.n == 1:
        return                                                                # (the single sequence is bound to Mirostat instead)
    if feat == "miro":
        for q in range(d.n):
            if miro_applies(q, d.n):
                dec_miro(d, q, MIRO[0] if on else 0.0, MIRO[1], MIRO[2], P + 1)
    else:
        switch_five(d, feat, on, banned)


def reference_miro(n_seq, feats):
    """a fresh decoder that has the requests before its first step and runs every step eagerly"""
    if n_seq == 1:
        feats = frozenset(feats - {"table", "cut"})
    if "miro" not in feats:
        return reference_fsm(n_seq, frozenset(feats))
    if (n_seq, feats) not in _REF:
        s = setup(n_seq)
        d = Dec(s["host"], s["cfg"], s["weights"], n_seq)
        d.o.set_fsm(pool(s["host"], s["cfg"].n_vocab))
        sample_all(d)
        for f in OTHERS + ("miro",):
            if f in feats:
                switch_any(d, f, True, s["banned"])
        _REF[(n_seq, feats)] = run_stage(d, s, "records" in feats, eager=True)
        d.o.close()
    return _REF[(n_seq, feats)]


@pytest.mark.parametrize("order", ORDERS, ids="-".join)
@pytest.mark.parametrize("n_seq", [1, 2, 16])
def test_mirostat_first_in_the_middle_and_last(hip, n_seq, order):
    s = setup(n_seq)
    d = Dec(s["host"], s["cfg"], s["weights"], n_seq)
    d.o.set_fsm(pool(s["host"], s["cfg"].n_vocab))
    sample_all(d)
    sampling_only = run_stage(d, s, False)
    same(sampling_only, reference(n_seq, frozenset()), "sampling")
    assert not d.o.mirostat_info()[3]
    assert reference_miro(n_seq, frozenset(["miro"]))[0].tolist() != sampling_only[0].tolist()        # (Mirostat moves ids)
    active = set()
    for on in (True, False):
        for feat in order:
            switch_any(d, feat, on, s["banned"])
            active ^= {feat}
            got = run_stage(d, s, "records" in active)
            same(got, reference_miro(n_seq, frozenset(active)), (feat, on, sorted(active)))
            assert d.o.mirostat_info()[3] == (on is False or "miro" in active)  # the rung stays once taken
    assert not active and got[0].tolist() == sampling_only[0].tolist()
    assert d.sampler_launches() == 1 and not d.o.mirostat_info()[0].any()
    # a binding alone samples nothing: with nobody sampling the step ends in the argmax, bound or not
    for q in range(n_seq):
        d.request(q, 0)
    dec_miro(d, 0, *MIRO, P + 1)
    assert d.sampler_launches() == 0
    dec_miro(d, 0, 0.0)
    same(run_stage(d, s, False), reference(n_seq, None), "nothing set, at the end")
    d.o.close()
