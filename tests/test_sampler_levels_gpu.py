"""-m gpu: the sampler's levels on one decoder.  A decoder's step ends in k_dec_argmax, or in the sampler kernel of
the latest feature it has ever used (tables, records, cuts); each first use drops the captured graphs once.  The feature tests meet
the features in the order they were built.  Here one decoder meets them in every order, switches them off again, and after every
change all its graph kinds must give what a fresh decoder with the same requests gives eagerly; and a sampled queue is served with
lanes sitting out, which runs the sampler's graphs of a subset of lanes."""
import itertools

import numpy as np
import pytest

from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from helpers import Q4, Q8, tiny_config
from test_bias_gpu import NINF, SEED, TOTAL, Dec, P
from test_logprobs_gpu import bits, dec_ask, dec_records
from test_model_gpu import host_cfg
from test_nucleus_gpu import dec_cut, dec_cut_info, model_setup
from test_serving_gpu import make_prompts

pytestmark = pytest.mark.gpu

FEATURES = ("table", "records", "cut")
N_TOP, CUT, TABLE = 3, (0.8, 0.1), 1
# positions P + 1 .. TOTAL - 1: a captured step, an eager step and four free-running steps (one replay of the DEC_GRAPH_STEPS graph)
# in turn, so every stage replays -- and, where the stage changed what a step ends in, captures -- both graph kinds
PATTERN = ["graph", "eager", "steps4", "graph", "steps4", "eager", "steps4", "graph", "eager", "steps4", "graph", "eager", "graph"]
assert sum(4 if p == "steps4" else 1 for p in PATTERN) == TOTAL - P - 1


def applies(feat, q, n_seq):
    """the table on the even sequences, records on every third, the cut on the odd ones; a single sequence has all three"""
    return n_seq == 1 or {"table": q % 2 == 0, "records": q % 3 == 0, "cut": q % 2 == 1}[feat]


def switch(d, feat, on, banned):
    if feat == "table" and on:
        d.o.set_bias_table(TABLE, [(j, NINF) for j in banned])
    for q in range(d.n):
        if not applies(feat, q, d.n):
            continue
        if feat == "table":
            assert d.bind_rc(q, TABLE if on else -1) == 0
        elif feat == "records":
            dec_ask(d, q, N_TOP if on else -1)
        else:
            dec_cut(d, q, *(CUT if on else (1.0, 0.0)))


def sample_all(d):
    for q in range(d.n):
        d.request(q, 40, 0.9, SEED, 3 * q + 1)


def run_stage(d, s, records, eager=False):
    """prompts in, teacher-forced with s["ids"], every position by PATTERN (eager: step by step without graphs); returns the ids
    [n_seq][positions], the records of the asking sequences and the last step's logits"""
    for q in range(d.n):
        d.prefill(q, s["prompts"][q])
        d.begin(q, s["ids"][q])
    n = P + 1
    for kind in PATTERN:
        if kind == "steps4" and not eager:
            d.o.decode_steps(n, 4)
        else:
            for i in range(4 if kind == "steps4" else 1):
                d.o.decode_step(n + i, use_graph=(kind == "graph" and not eager))
        n += 4 if kind == "steps4" else 1
    assert n == TOTAL
    ids = np.array([[d.result(q, n) for n in range(P + 1, TOTAL)] for q in range(d.n)])
    rec = {q: dec_records(d, q, P + 1, TOTAL - P - 1, N_TOP) for q in range(d.n) if records and applies("records", q, d.n)}
    return ids, rec, np.stack([d.logits(q) for q in range(d.n)])


_SETUP, _REF = {}, {}


def setup(n_seq):
    """model, prompts, the ids every run is teacher-forced with (the greedy ids of a first run) and the table's banned half"""
    if n_seq not in _SETUP:
        host = load_package().load_host()
        cfg, weights = model_setup(host, n_vocab=512, max_ctx=64)
        V = cfg.n_vocab
        prompts = [list(host.synthetic_tokens(P, seed=700 + q, n_vocab=V)) for q in range(n_seq)]
        d = Dec(host, cfg, weights, n_seq)
        ids = [d.o.generate(prompts[0], TOTAL)] if d.one else d.o.generate(prompts, TOTAL)
        d.o.close()
        early = sorted({int(g[p]) for g in ids for p in (P, P + 1, P + 2)})            # what the greedy run produces first, then the lowest ids
        banned = (early + [j for j in range(V) if j not in early])[: V // 2]
        _SETUP[n_seq] = dict(host=host, cfg=cfg, weights=weights, prompts=prompts, ids=ids, banned=sorted(banned))
    return _SETUP[n_seq]


def reference(n_seq, feats):
    """a fresh decoder that has the requests before its first step and runs every step eagerly; feats None: nothing set at all,
    otherwise every sequence samples and the features of the set are on.  Nine per n_seq, shared by the six orders."""
    if (n_seq, feats) not in _REF:
        s = setup(n_seq)
        d = Dec(s["host"], s["cfg"], s["weights"], n_seq)
        if feats is not None:
            sample_all(d)
            for f in FEATURES:
                if f in feats:
                    switch(d, f, True, s["banned"])
        _REF[(n_seq, feats)] = run_stage(d, s, feats is not None and "records" in feats, eager=True)
        d.o.close()
    return _REF[(n_seq, feats)]


def same(got, want, what):
    ids, rec, logits = got
    wids, wrec, wlogits = want
    assert ids.tolist() == wids.tolist(), what
    assert sorted(rec) == sorted(wrec), what
    for q in rec:
        for a, b in zip(rec[q], wrec[q]):
            assert (bits(a) == bits(b)).all() if a.dtype == np.float32 else a.tolist() == b.tolist(), (what, q)
    assert (bits(logits) == bits(wlogits)).all(), what


@pytest.mark.parametrize("order", list(itertools.permutations(FEATURES)), ids="-".join)
@pytest.mark.parametrize("n_seq", [1, 2, 16])
def test_features_in_any_order_of_first_use(hip, n_seq, order):
    """eight stages on one decoder -- nothing set, every sequence sampling, the three features on one by one in `order`, off one by
    one in the same order -- each equal to the fresh eager decoder: ids, record bits, logits bits"""
    s = setup(n_seq)
    d = Dec(s["host"], s["cfg"], s["weights"], n_seq)
    same(run_stage(d, s, False), reference(n_seq, None), "nothing set")
    assert d.sampler_launches() == 0
    sample_all(d)
    sampling_only = run_stage(d, s, False)
    same(sampling_only, reference(n_seq, frozenset()), "sampling")
    # (the stages are not one and the same: sampling moves ids off the greedy ones, the table and the cut move them again)
    assert sampling_only[0].tolist() != reference(n_seq, None)[0].tolist()
    for feat in ("table", "cut"):
        assert reference(n_seq, frozenset([feat]))[0].tolist() != sampling_only[0].tolist(), feat
    active = set()
    for on in (True, False):
        for feat in order:
            switch(d, feat, on, s["banned"])
            active ^= {feat}
            got = run_stage(d, s, "records" in active)
            same(got, reference(n_seq, frozenset(active)), (feat, on, sorted(active)))
    # every feature off again, the sequences still sample: the sampling-only ids, from one sampler launch per lane; the decoder
    # stays on the cut's rung, and no sequence is bound or asks any more
    assert not active and got[0].tolist() == sampling_only[0].tolist()
    assert d.sampler_launches() == 1
    assert dec_cut_info(d)[3]
    if not d.one:
        _, tables, until = d.o.bias_info()
        assert (tables == -1).all() and (until == 0).all()
    # (a request is read back per sequence only through a decoder handle, which the host objects keep to themselves: what every
    #  sequence reads as is shown by the step itself -- with nobody sampling either, it ends in the argmax again)
    for q in range(n_seq):
        d.request(q, 0)
    assert d.sampler_launches() == 0
    same(run_stage(d, s, False), reference(n_seq, None), "nothing set, at the end")
    d.o.close()


def test_a_sampled_queue_with_lanes_sitting_out(hip):
    """test_serving_gpu.test_lanes_without_a_live_slot_sit_the_run_out under the sampler: a queue through 256 slots (two lanes) with
    and without lane skipping and through 16 slots, two prompts of three drawing top-k 40, the third greedy.  The same ids per prompt;
    the skipping run left a lane out, so it replayed the sampler's graphs of a subset of lanes."""
    host = load_package().load_host()
    cfg = host_cfg(tiny_config(Q4, Q8, n_heads=4, n_kv_heads=2, max_ctx=128, n_layers=2))
    weights = [host.synth_weight(cfg, 1414, i) for i in range(len(cfg.weight_shapes()))]
    n = 140
    prompts = make_prompts(host, cfg, [8 + (23 * i) % 63 for i in range(n)], 17)
    budgets = np.array([4 + (11 * i) % 31 for i in range(n)], np.int32)
    ks = [0 if j % 3 == 2 else 40 for j in range(n)]
    outs, stats = [], []
    try:
        for slots, skip in ((256, True), (256, False), (16, True)):
            hip.set_lane_skip(skip)
            b = host.batch(cfg, slots)
            for i, w in enumerate(weights):
                b.set_weight(i, w)
            got, st = b.serve_topk(prompts, 128, -1, ks, 0.9, SEED, slice_steps=8, max_new_each=budgets)
            assert st["admissions"] == n
            outs.append(got); stats.append(st)
            b.close()
    finally:
        hip.set_lane_skip(False)
    print("lane-steps with / without skipping:", stats[0]["lane_steps"], stats[1]["lane_steps"], "steps", stats[0]["steps"], stats[1]["steps"])
    for j in range(n):
        assert len(outs[0][j]) == len(prompts[j]) + budgets[j], j
        assert outs[0][j].tolist() == outs[1][j].tolist() == outs[2][j].tolist(), j
    assert stats[0]["lane_steps"] < 2 * stats[0]["steps"], stats[0]
