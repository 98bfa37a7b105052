"""bench.py on one GPU at a small shape: a plain run prints the headline keys and nothing else, --full adds the rest, and the
two runs' last timed steps return the same arrays (the timed path does not depend on --full)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--steps", "2", "--warmup", "1", "--templates", "600", "--batch", "8", "--version", "vits14-reg", "--layer", "9", "--size", "224"]
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup", "scaling", "vs_baseline",
            "config", "ranks_seen", "full"}


def run_bench(extra, dump_dir):
    env = dict(os.environ, FP_CPU_BASELINE_ALL_CORES="0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, "--dump-outputs", str(dump_dir), *extra]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line"
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_full_adds_the_rest(tmp_path):
    plain = run_bench([], tmp_path / "plain")
    assert set(plain) == HEADLINE, sorted(set(plain) ^ HEADLINE)
    assert plain["full"] is False and plain["higher_is_better"] is True and plain["dtype"] == "bf16" and plain["unit"] == "detections/s"
    assert plain["steps"] == 2 and plain["warmup"] == 1 and plain["n_gpus"] == 1 and plain["ranks_seen"] == 1
    assert plain["value"] > 0 and abs(plain["value"] - 8 * 2 / (plain["ms_per_step"] * 2 / 1e3)) < 0.02 * plain["value"]

    full = run_bench(["--full", "--cpu-detections", "1", "--other-configs", "none"], tmp_path / "full")
    assert full["full"] is True and HEADLINE <= set(full)
    assert {k: full[k] for k in ("metric", "unit", "higher_is_better", "dtype", "config")} == {k: plain[k] for k in ("metric", "unit", "higher_is_better", "dtype", "config")}
    for key in ("roofline", "tie_order_cost", "token_selection", "parity", "parity_mode", "cpu_baseline", "latency_b1", "pipeline"):
        assert key in full, key
    assert full["parity"]["planted"]["planted_top1"] == 8

    names = sorted(os.listdir(tmp_path / "plain"))
    assert "template_id.npy" in names and names == sorted(os.listdir(tmp_path / "full"))
    for name in names:   # same inputs, same timed path: the same results, bit for bit
        a, b = np.load(tmp_path / "plain" / name), np.load(tmp_path / "full" / name)
        assert a.shape == b.shape and np.array_equal(a, b), name
