"""bench.py's command line: a plain run prints exactly one result line and does none of the
extra measurements (those belong to ``--full``), ``--steps`` sets the number of timed steps,
and ``--dump-outputs DIR`` writes what the last timed step computed - identically from run
to run of one build, so two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _run(tmp_path, args, timeout=300):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MPA_BENCH_INJECT"):
        env.pop(k, None)
    env["MASTER_ADDR"] = "127.0.0.1"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(args)
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return [json.loads(l) for l in r.stdout.splitlines() if l.strip().startswith("{")]


def _check_dump(rec, out, steps):
    assert rec["steps"] == steps
    assert all(k in rec for k in HEADLINE_KEYS)
    assert rec["unit"] == "images/sec" and rec["higher_is_better"] is True
    assert rec["ms_per_step"] > 0
    # value and ms_per_step describe the same timed steps
    per_step = rec["config"]["global_batch"] / (rec["ms_per_step"] * 1e-3)
    assert rec["value"] == pytest.approx(per_step, rel=1e-2)
    for k in ("small_batch", "multi_gpu"):
        assert k not in rec
    assert "hbm_probe_at_start_gbps" not in rec["host"]
    arrays = {n: np.load(str(out / (n + ".npy"))) for n in ("loss", "grads", "params")}
    assert sorted(p.name for p in out.iterdir()) == ["grads.npy", "loss.npy", "params.npy"]
    total = 0
    for n, a in arrays.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), n
        assert list(a.shape) == rec["dumped_outputs"]["shapes"][n]
        total += a.nbytes
    assert total <= 64 * 2**20
    assert arrays["loss"].shape == (1,) and arrays["loss"][0] > 0
    assert np.abs(arrays["grads"]).sum() > 0 and np.abs(arrays["params"]).sum() > 0
    return arrays


def test_plain_cpu_run_is_one_line_and_dumps_reproducible_outputs(tmp_path):
    args = ["--device", "cpu", "--image-size", "32", "--batch", "2", "--classes", "10",
            "--steps", "2", "--warmup", "1"]
    runs = []
    for tag in ("a", "b"):
        out = tmp_path / tag
        recs = _run(tmp_path, args + ["--dump-outputs", str(out)])
        assert len(recs) == 1
        runs.append(_check_dump(recs[0], out, 2))
    for n in runs[0]:  # host ops, one thread pool: bitwise equal from run to run
        assert np.array_equal(runs[0][n], runs[1][n]), n


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_bench_under_test",
                                                  os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_pace_waits_for_the_step_max_lead_earlier():
    """The host may be MAX_LEAD steps ahead of the device and no more: step n waits for
    the event of step n - MAX_LEAD, in order, and for nothing newer."""
    bench = _bench_module()
    made, waited = [], []

    class Ev:
        def __init__(self):
            self.recorded = False
            made.append(self)

        def record(self):
            self.recorded = True

        def synchronize(self):
            assert self.recorded
            waited.append(made.index(self))

    pace = bench._Pace("cuda", event_factory=Ev)
    lead = pace.MAX_LEAD
    assert 1 <= lead <= 16  # (each step ahead holds its stream-crossing tensors)
    for n in range(3 * lead):
        pace.step()
        assert waited == list(range(max(0, n + 1 - lead)))
    assert len(pace._events) == lead
    cpu = bench._Pace("cpu", event_factory=Ev)
    cpu.step()
    assert len(made) == 3 * lead  # host runs are synchronous: no events


def test_dump_samples_large_arenas_at_fixed_indices(tmp_path, monkeypatch):
    """An arena above the element cap is sampled: same sorted indices every time."""
    import torch
    bench = _bench_module()
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 100)

    class Arena:
        grad = torch.arange(50, dtype=torch.float32)
        master = torch.arange(1000, dtype=torch.float64)

    for tag in ("a", "b"):
        shapes = bench._dump_outputs(str(tmp_path / tag), torch.tensor(2.5), Arena)
        assert shapes == {"loss": [1], "grads": [50], "params": [100]}
    a, b = (np.load(str(tmp_path / t / "params.npy")) for t in ("a", "b"))
    assert a.dtype == np.float32 and np.array_equal(a, b)
    assert (np.diff(a) >= 0).all() and 0 <= a.min() and a.max() < 1000
    assert np.array_equal(np.load(str(tmp_path / "a" / "grads.npy")), np.arange(50))
    assert np.load(str(tmp_path / "a" / "loss.npy"))[0] == 2.5


@pytest.mark.gpu
def test_plain_gpu_run_is_one_line_and_dumps_outputs(gpu, tmp_path):
    """Two processes, same arguments: a dumping run is made in deterministic mode, so
    after several optimizer steps every dumped array is bitwise the same (several blocks
    per BN reduction and per GEMM at this size: 48 x 64 x 64 images)."""
    args = ["--batch", "48", "--image-size", "64", "--classes", "1000", "--steps", "4",
            "--warmup", "2", "--reserve-gib", "0"]
    runs = []
    for tag in ("a", "b"):
        out = tmp_path / tag
        recs = _run(tmp_path, args + ["--dump-outputs", str(out)])
        assert len(recs) == 1
        assert recs[0]["dtype"] == "bf16" and recs[0]["n_gpus"] == 1
        assert recs[0]["config"]["deterministic"] is True
        runs.append(_check_dump(recs[0], out, 4))
    for n in runs[0]:
        assert np.array_equal(runs[0][n], runs[1][n]), n


@pytest.mark.gpu
def test_plain_gpu_run_without_dump_keeps_the_default_mode(gpu, tmp_path):
    recs = _run(tmp_path, ["--batch", "32", "--image-size", "64", "--classes", "1000",
                           "--steps", "2", "--warmup", "1", "--reserve-gib", "0"])
    assert len(recs) == 1 and recs[0]["config"]["deterministic"] is False
    assert "dumped_outputs" not in recs[0] and "small_batch" not in recs[0]
