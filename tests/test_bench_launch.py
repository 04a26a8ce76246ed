"""CPU suite: `python bench.py --gpus N` as the driver invokes it (no launcher around it) must start its N ranks itself, relay rank 0's
JSON line and return the children's code.  Driven here with BENCH_REHEARSAL=stub: gloo children, the sweep replaced by a stub (the
launch / rank / reduction logic of bench.py is what runs; nothing of the path is computed and the line says so)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra_env, *argv, timeout=300):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(extra_env)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=env, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("n", [2, 3])
def test_bench_starts_its_own_ranks(n):
    r = _run({"BENCH_REHEARSAL": "stub"}, "--gpus", str(n), "--steps", "5", "--warmup", "1", "--no-cpu")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == n and out["steps"] == 5 and out["warmup"] == 1 and out["scaling"] == "weak"
    assert out["config"]["latents_total"] == 4096 * n
    assert out["nll_total"] == 4096.0 * n                     # every rank's stub total, summed by the pass's all-reduce
    assert "stub" in out["rehearsal"]


def test_bench_reports_a_failing_rank():
    # ranks that fail after their process group is up (c3loop refuses --dump-outputs, with or without a GPU on the box): the children
    # fail, the parent must not exit 0 or print a line
    r = _run({"BENCH_REHEARSAL": "stub"}, "--gpus", "2", "--steps", "2", "--warmup", "0", "--config", "c3loop", "--dump-outputs", "unused",
             timeout=300)
    assert r.returncode != 0
    assert not [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]


def test_bench_refuses_a_world_size_mismatch():
    r = _run({"BENCH_REHEARSAL": "stub", "WORLD_SIZE": "1", "RANK": "0"}, "--gpus", "2", "--steps", "1")
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stderr + r.stdout)


def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    # a plain run carries the headline only and writes the last timed step's outputs; --full adds the figures that take runs of their own
    import numpy as np
    r = _run({"BENCH_REHEARSAL": "stub"}, "--gpus", "1", "--steps", "7", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")][-1])
    assert out["steps"] == 7 and out["ms_per_step"] > 0 and out["unit"] == "Kalman steps/s" and out["higher_is_better"] is True
    assert "roofline" not in out and "cpu_baseline" not in out and "other_configs" not in out
    files = sorted(p.name for p in tmp_path.iterdir())
    assert files == ["nll.npy", "nll_total.npy", "x.npy", "yhat.npy"], files
    arrays = [np.load(tmp_path / f) for f in files]
    assert all(a.dtype in (np.float32, np.float64) for a in arrays)
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= 64 * 10 ** 6
    r = _run({"BENCH_REHEARSAL": "stub"}, "--gpus", "1", "--steps", "2", "--warmup", "0", "--full")
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")][-1])
    assert out["steps"] == 2 and "roofline" in out and "ms_per_step_with_event_pairs" in out
