"""-m gpu: the command line's --score (host/tinyllama_cli.cpp): windows of at most --ctx ids, each [1] + the next ctx - 1
text ids, scored through score_many -- the same numbers as the Python binding over the same windows."""
import math
import subprocess

import numpy as np
import pytest

from gpu_common import hip  # noqa: F401
from __graft_entry__ import load_package
from test_cli_gpu import write_vocab

pytestmark = pytest.mark.gpu


def test_cli_score_matches_score_many(hip, tmp_path):
    pkg = load_package()
    host = pkg.load_host()
    cfg = host.default_config(4, 3)                       # full-size TinyLlama, q4 weights x q8 activations
    ckpt, vocab, text_path = str(tmp_path / "tinyllama.q4.gten"), str(tmp_path / "vocab.bin"), str(tmp_path / "text.txt")
    host.write_gten(cfg, 5151, ckpt)
    write_vocab(vocab)
    r = np.random.default_rng(3)
    letters = "abcdefghijklmnopqrstuvwxyz"
    words = ["".join(r.choice(list(letters), int(r.integers(1, 8)))) for _ in range(900)]
    text = " ".join(words) + "\nhello world\n"
    with open(text_path, "w") as f:
        f.write(text)
    tok = host.tokenizer(vocab)
    ids = tok.encode(text, chat_template=False)
    assert 2500 <= len(ids) <= 6000, len(ids)
    ctx = 1024
    res = subprocess.run([pkg.build.HOST_CLI, "-q4", "--score", text_path, "--ctx", str(ctx), "--ids", "--model", ckpt, "--tokenizer", vocab],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.strip().splitlines()
    final = lines[-1]
    assert final.startswith("score: "), final
    fields = dict(kv.split("=") for kv in final[len("score: "):].split())
    assert int(fields["tokens"]) == len(ids)
    per_id = [ln.split() for ln in lines[:-1]]
    assert len(per_id) == len(ids) and [int(p[0]) for p in per_id] == list(ids)

    windows = [[1] + list(ids[i:i + ctx - 1]) for i in range(0, len(ids), ctx - 1)]
    assert len(windows) >= 3 and len(windows[-1]) < ctx
    cfg2 = host.default_config(4, 3)
    cfg2.max_ctx = ctx                                   # the CLI builds TinyLlama{ctx, dtype} for --score
    m = host.model(cfg2)
    m.load_gten(ckpt)
    lp, rk = m.score_many(windows)
    m.close()
    lps = np.concatenate([w[:-1] for w in lp]).astype(np.float64)
    rks = np.concatenate([w[:-1] for w in rk])
    assert all(w[-1] == 0 for w in lp)
    nll = -lps.mean()
    assert f"{nll:.9g}" == fields["nll"], (nll, fields["nll"])
    assert abs(float(fields["ppl"]) - math.exp(nll)) <= 1e-6 * math.exp(nll)
    assert abs(float(fields["greedy"]) - float((rks == 0).mean())) <= 1e-9
    assert [int(p[2]) for p in per_id] == rks.tolist()
