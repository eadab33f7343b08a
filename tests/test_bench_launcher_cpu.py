"""not gpu: `python bench.py --gpus N` really starts N replicas (round-1 verdict: the flag was parsed and ignored).

bench.py runs here with `--engine stub`: a sleeping stand-in for the decoder, NO GPU and no arithmetic, so what these
tests exercise is the launcher (tinyllama.cpp_amd/replicas.py launch(): one worker per GPU, the environment
torch.distributed.run would set), the rendezvous (gloo), the barrier-bracketed timed region with MAX over ranks, the
per-rank / solo / efficiency bookkeeping and the ONE JSON line of rank 0 -- the same code the GPU run takes."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def run_bench(*extra, env=None, timeout=300):
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, BENCH, "--engine", "stub", "--steps", "12", "--warmup", "2", *extra],
                          capture_output=True, text=True, env=e, timeout=timeout)


def result_line(proc):
    lines = [l for l in proc.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, proc.stdout + proc.stderr          # ONE JSON line
    return json.loads(lines[0])


@pytest.mark.parametrize("n", [2, 4])
def test_gpus_n_starts_n_replicas(n):
    p = run_bench("--gpus", str(n))
    assert p.returncode == 0, p.stderr[-2000:]
    r = result_line(p)
    assert r["n_gpus"] == n and r["steps"] == 12 and r["warmup"] == 2
    assert r["metric"].startswith("STUB") and f"{n} GPUs" in r["metric"]
    assert [x["rank"] for x in r["per_rank"]] == list(range(n))
    # value = tokens of all ranks / the slowest rank's time: the stub's higher ranks are slower, so the aggregate is
    # below the sum of the per-rank rates and at least n x the slowest rank's rate
    rates = [x["tok_s"] for x in r["per_rank"]]
    assert min(rates) * n <= r["value"] * 1.02 and r["value"] <= sum(rates) * 1.02
    assert rates[0] >= rates[-1]
    assert abs(r["value"] - 12 * n / (r["ms_per_step"] * 12e-3)) / r["value"] < 0.02
    assert 0.3 < r["efficiency"] <= 1.1 and abs(r["efficiency"] - r["value"] / (n * r["solo_rank0_tok_s"])) < 1e-3
    assert r["launcher"]["kind"].startswith("bench.py")
    assert r["config"]["parallelism"] == f"replicas x{n}"


def test_gpus_1_line_is_the_single_replica_line():
    p = run_bench("--gpus", "1")
    assert p.returncode == 0, p.stderr[-2000:]
    r = result_line(p)
    assert r["n_gpus"] == 1 and "per_rank" not in r and "efficiency" not in r and "launcher" not in r
    assert "1 GPU;" in r["metric"]


def test_a_failing_replica_fails_the_run():
    p = run_bench("--gpus", "2", env={"GTEN_BENCH_STUB_FAIL_RANK": "1"})
    assert p.returncode != 0
    assert not [l for l in p.stdout.splitlines() if l.startswith("{")]


def test_curve_reports_smaller_replica_counts():
    p = run_bench("--gpus", "4", "--curve")
    assert p.returncode == 0, p.stderr[-2000:]
    r = result_line(p)
    assert [c["n_gpus"] for c in r["scaling_curve"]] == [1, 2, 4]
    assert r["scaling_curve"][-1]["value"] == r["value"]
    assert r["scaling_curve"][0]["efficiency_vs_1gpu_run"] == 1.0


def test_same_worker_under_torch_distributed_run():
    """the driver's own form: python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N"""
    sys.path.insert(0, os.path.join(ROOT, "tinyllama.cpp_amd"))
    import importlib.util
    spec = importlib.util.spec_from_file_location("gten_replicas_t", os.path.join(ROOT, "tinyllama.cpp_amd", "replicas.py"))
    rep = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rep)
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "TORCHELASTIC_RUN_ID")}
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(rep.free_port()), BENCH, "--gpus", "2",
                        "--engine", "stub", "--steps", "12", "--warmup", "2"], capture_output=True, text=True, env=e, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    r = result_line(p)
    assert r["n_gpus"] == 2 and len(r["per_rank"]) == 2 and "launcher" not in r


@pytest.mark.parametrize("n", [2, 4])
def test_one_global_prompt_queue_is_sharded_over_the_replicas(n):
    """north_star's multi-GPU split: `--gpus N` ranks take replicas.shard_prompts(n_prompts, rank, N) of ONE global queue
    through their own slots; the N > 1 line carries the aggregate serving rate beside the batch-1 rate, and every prompt
    is served exactly once (an all-reduced counter per prompt)"""
    p = run_bench("--gpus", str(n), "--serve", "24", "--full")
    assert p.returncode == 0, p.stderr[-2000:]
    r = result_line(p)
    sv = r["sharded_serving"]
    assert sv["prompts"] == 24 * n and sv["prompts_per_rank"] == [24] * n
    assert sv["every_prompt_served_exactly_once"] is True
    assert [x["rank"] for x in sv["per_rank"]] == list(range(n))
    assert sum(x["new_tokens"] for x in sv["per_rank"]) == sv["new_tokens"] > 0
    assert abs(sv["new_tok_s"] - sv["new_tokens"] / sv["wall_s"]) / sv["new_tok_s"] < 0.02
    assert sv["wall_s"] >= max(x["wall_s"] for x in sv["per_rank"]) - 1e-3
    assert r["value"] > 0 and r["config"]["parallelism"] == f"replicas x{n}"        # the batch-1 rate is still the headline


@pytest.mark.parametrize("n", [2, 8])
def test_batched_aggregates_sit_at_the_top_level_with_their_own_efficiency(n):
    """round-4 verdict: at N GPUs `value` is N x batch-1 (BASELINE.json's metric) while one GPU does ~40 x that batched -- the N > 1
    line carries the aggregate of the batched step (every replica its own 256 sequences) and of the sharded serving queue at the
    top level, each with an efficiency against rank 0 alone, measured in the same run.  World 8 is the driver's SCALE run."""
    p = run_bench("--gpus", str(n), "--serve", "16", "--full", timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    r = result_line(p)
    assert r["n_gpus"] == n and len(r["per_rank"]) == n
    bd, sv = r["batched_decode"], r["sharded_serving"]
    assert [x["rank"] for x in bd["per_rank"]] == list(range(n)) and bd["steps"] == 12
    assert r["batched_tok_s"] == bd["tok_s"] > 0 and r["batched_efficiency"] == bd["efficiency"]
    assert r["serving_new_tok_s"] == sv["new_tok_s"] > 0 and r["serving_efficiency"] == sv["efficiency"]
    # tokens of all ranks / the slowest rank's time; the stub's higher ranks are slower, so the efficiency is below 1 and above
    # the slowest rank's share
    rates = [x["tok_s"] for x in bd["per_rank"]]
    assert min(rates) * n <= bd["tok_s"] * 1.03 and bd["tok_s"] <= sum(rates) * 1.03
    assert abs(bd["efficiency"] - bd["tok_s"] / (n * bd["solo_rank0_tok_s"])) < 2e-3 and 0.2 < bd["efficiency"] <= 1.1
    assert abs(sv["efficiency"] - sv["new_tok_s"] / (n * sv["solo_rank0_new_tok_s"])) < 2e-3 and 0.05 < sv["efficiency"] <= 1.2
    assert sv["every_prompt_served_exactly_once"] is True and sv["prompts_per_rank"] == [16] * n
    assert r["value"] > 0 and r["efficiency"] > 0                                      # the batch-1 headline and its efficiency stay


def test_a_lost_request_is_reported():
    p = run_bench("--gpus", "2", "--serve", "24", "--full", env={"GTEN_BENCH_STUB_DROP_RANK": "1"})
    assert p.returncode == 0, p.stderr[-2000:]
    assert result_line(p)["sharded_serving"]["every_prompt_served_exactly_once"] is False


def test_brief_runs_skip_the_sharded_queue():
    p = run_bench("--gpus", "2", "--full", "--brief")
    assert p.returncode == 0, p.stderr[-2000:]
    r = result_line(p)
    assert "sharded_serving" not in r and "batched_decode" not in r


def test_plain_runs_time_only_the_headline():
    """without --full a run does only what `value` needs: no roofline, no secondary or N > 1 legs, no CPU baseline"""
    for n in (1, 2):
        p = run_bench("--gpus", str(n), "--serve", "16")
        assert p.returncode == 0, p.stderr[-2000:]
        r = result_line(p)
        assert r["steps"] == 12 and r["ms_per_step"] > 0 and r["value"] > 0 and r["roofline"] is None
        assert not {"sharded_serving", "batched_decode", "cpu_baseline", "multi_stream", "serving", "prefill"} & set(r)


def test_dump_outputs_writes_the_timed_steps_ids(tmp_path):
    import numpy as np
    got = []
    for k in (1, 2):
        d = tmp_path / str(k)
        p = run_bench("--gpus", "1", "--dump-outputs", str(d))
        assert p.returncode == 0, p.stderr[-2000:]
        ids = np.load(d / "step_ids.npy")
        assert ids.dtype == np.float64 and ids.shape == (12,)
        assert int(ids[-1]) == result_line(p)["config"]["last_token"]
        got.append(ids)
    assert np.array_equal(got[0], got[1])                  # seeded inputs: the same arguments, the same outputs


def test_shards_partition_the_queue():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gten_replicas_s", os.path.join(ROOT, "tinyllama.cpp_amd", "replicas.py"))
    rep = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rep)
    for n_prompts in (0, 1, 7, 256, 1000):
        for world in (1, 2, 3, 8):
            shards = [rep.shard_prompts(n_prompts, r, world) for r in range(world)]
            assert sorted(j for sh in shards for j in sh) == list(range(n_prompts))
            assert max(len(sh) for sh in shards) - min(len(sh) for sh in shards) <= 1


def test_source_fingerprint_ignores_comments_not_code():
    """profiles/traffic.json is tied to the kernels by bench.csrc_fingerprint(): a note added to a kernel source must not
    orphan the counters collected on it, any change of code (or of a string / character literal) must"""
    import bench
    a = 'int a = 1; // note "x"\n/* block\n comment */ const char* s = "http://x // not a comment"; char c = \'"\';\n#define M(x) x // tail\n'
    b = 'int a = 1;\nconst char* s = "http://x // not a comment";   char c = \'"\';   /* other words */\n#define M(x) x\n'
    assert bench.code_only(a) == bench.code_only(b)
    assert bench.code_only(a) != bench.code_only(a.replace("a = 1", "a = 2"))
    assert bench.code_only(a) != bench.code_only(a.replace("// not a comment", "// NOT a comment"))
    assert "note" not in bench.code_only(a) and "block" not in bench.code_only(a)
    assert len(bench.csrc_fingerprint()) == 16
