"""bench.py's host logic on the CPU: the schedule bookkeeping of the timed PC iterations, --dump-outputs and what a plain run and a --full run measure."""
import os
import sys

import numpy as np
import pytest
import torch

import _util

sys.path.insert(0, _util.ROOT)
import bench  # noqa: E402


class _StubEngine:
    """records what the runner asks of a sampler engine: resets and the step index of every iteration"""

    def __init__(self):
        self.step, self.resets, self.iterations = 0, 0, []

    def reset(self, x):
        self.step, self.resets = 0, self.resets + 1

    def run_steps(self, prog, steps, use_graph=True):
        for _ in range(steps):
            self.iterations.append(self.step)
            self.step += 1


def test_schedule_runner_keeps_the_step_index_inside_the_schedule():
    eng = _StubEngine()
    r = bench.ScheduleRunner(eng, None, None, N=7, use_graph=True)
    r.run(3)
    for _ in range(4):
        r.run(5)                                    # pre-warm chunks run past the end of the schedule
    assert max(eng.iterations) == 6 and eng.resets == 3 and eng.step == r.pos
    r.restart()
    eng.iterations.clear()
    r.run(16)                                       # timed steps: the schedule from its first iteration, as often as it takes
    assert eng.iterations == list(range(7)) + list(range(7)) + [0, 1]
    assert len(eng.iterations) == 16


def test_bench_rejects_steps_below_one_and_dumps_outside_the_sampler():
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse(["--dump-outputs", "out", "--train-only"])
    with pytest.raises(SystemExit):
        bench.parse(["--dump-outputs", "out", "--workload", "subvp_ode"])
    assert bench.parse(["--dump-outputs", "out", "--steps", "4"]).dump_outputs == "out"


LEGS = ("no_roofline", "no_cpu_baseline", "no_train", "no_other_matrix", "no_extras", "no_exchange_probe", "no_telemetry")


def test_a_plain_bench_run_times_the_headline_alone_and_full_measures_the_rest():
    plain = bench.parse(["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert not plain.full and all(getattr(plain, k) for k in LEGS)
    assert (plain.steps, plain.warmup, plain.prewarm_s, plain.batch, plain.sde_steps) == (5, 2, 3.0, 256, 1000)
    full = bench.parse(["--gpus", "1", "--steps", "5", "--warmup", "2", "--full"])
    assert full.full and not any(getattr(full, k) for k in LEGS)
    some = bench.parse(["--full", "--no-train", "--no-extras"])
    assert some.no_train and some.no_extras and not (some.no_roofline or some.no_cpu_baseline or some.no_other_matrix)
    # the per-kernel lists come from the roofline legs
    for opt in ("--dump-ops", "--dump-train-ops"):
        with pytest.raises(SystemExit):
            bench.parse([opt, "ops.json"])
        assert getattr(bench.parse([opt, "ops.json", "--full"]), opt[2:].replace("-", "_")) == "ops.json"


def test_dump_outputs_writes_float32_arrays(tmp_path):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(4, 3, 8, 8, generator=g)
    shapes = bench.dump_outputs(str(tmp_path / "d"), {"x": x, "x_mean": x.double(), "n": np.arange(3)})
    assert shapes == {"x": [4, 3, 8, 8], "x_mean": [4, 3, 8, 8], "n": [3]}
    got = {k: np.load(os.path.join(str(tmp_path / "d"), k + ".npy")) for k in shapes}
    assert got["x"].dtype == np.float32 and np.array_equal(got["x"], x.numpy())
    assert got["x_mean"].dtype == np.float64 and got["n"].dtype == np.float32


def test_dump_outputs_samples_above_the_budget_the_same_way_every_time(tmp_path):
    a = np.arange(1000, dtype=np.float32)
    b = -np.arange(3000, dtype=np.float32).reshape(30, 100)
    budget = 2000                                   # bytes: a quarter of a's share and of b's
    s1 = bench.dump_outputs(str(tmp_path / "1"), {"a": a, "b": b}, budget=budget)
    s2 = bench.dump_outputs(str(tmp_path / "2"), {"a": a, "b": b}, budget=budget)
    assert s1 == s2 == {"a": [125], "b": [375]}
    total = 0
    for k in s1:
        v1, v2 = np.load(str(tmp_path / "1" / (k + ".npy"))), np.load(str(tmp_path / "2" / (k + ".npy")))
        assert np.array_equal(v1, v2) and len(np.unique(v1)) == v1.size
        total += v1.nbytes
    assert total <= budget
    assert np.all(np.diff(np.load(str(tmp_path / "1" / "a.npy"))) > 0)          # sorted indices: the sample keeps the order
