"""bench.py's two kinds of run: a plain one does only what the headline needs (set-up, warm-up, the timed steps,
--dump-outputs, the line); `--full` adds the further regions and sustained steps, the roofline, the oracle check, the
CPU baseline and the legs outside the timed region."""
import json
import os
import subprocess
import sys

import pytest

from tests.test_bench_rank_record import ROOT, _bench

HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY_KEYS = ("value_median_of_5", "all_regions_ms_per_step", "sustained", "roofline", "cpu_baseline",
                  "speedup_vs_cpu_port", "cpu_quota_cpus", "latency_case", "product_point", "roofline_pair",
                  "roofline_editdist", "e2e", "e2e_sharded", "e2e_samples", "e2e_cohort")


def test_full_is_an_option_and_off_by_default(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert bench.parse().full is True


def _run(args, timeout):
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert res.returncode == 0, res.stderr[-4000:]
    lines = res.stdout.strip().splitlines()
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.spawns_gpu_children
def test_plain_run_prints_the_headline_and_nothing_that_needs_runs_of_its_own(tmp_path):
    small = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--samples", "8"]
    r = _run(small + ["--dump-outputs", str(tmp_path / "plain")], 300)
    for k in HEADLINE_KEYS:
        assert k in r, k
    assert r["steps"] == 3 and r["warmup"] == 1 and r["value"] > 0 and r["ms_per_step"] > 0
    assert r["value"] == pytest.approx(r["config"]["ops_per_step_per_gpu"] / (r["ms_per_step"] * 1e-3), rel=1e-9)
    assert not [k for k in FULL_ONLY_KEYS if k in r]
    assert list(r)[-1] == "summary" and r["summary"] == {"value": r["value"], "ms_per_step": r["ms_per_step"]}
    assert os.path.exists(str(tmp_path / "plain" / "sig_aln.npy"))
    # --full: the same headline fields, and beside them what takes runs of its own (the legs of --no-extras aside)
    f = _run(small + ["--full", "--no-extras", "--cpu-seconds", "0.5"], 600)
    for k in HEADLINE_KEYS + ("value_median_of_5", "all_regions_ms_per_step", "sustained", "roofline", "cpu_baseline",
                              "cpu_quota_cpus"):
        assert k in f, k
    assert len(f["all_regions_ms_per_step"]) == 5 and f["sustained"]["steps"] == 200
    assert f["roofline"]["kernel_ms"] > 0 and f["cpu_baseline"]["value"] > 0
    assert f["config"]["ops_per_step_per_gpu"] == r["config"]["ops_per_step_per_gpu"]
    assert list(f)[-1] == "summary" and "e2e_wall_s" in f["summary"]
