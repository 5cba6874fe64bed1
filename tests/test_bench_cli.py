"""CPU checks of bench.py's output dump: what a caller of the timed path receives, population by
population, as float64 .npy files, and a fixed, seeded sample of the populations when that would
exceed the size limit.  (The plain and --full runs themselves: tests/test_bench_gpu.py.)"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Solution:
    def __init__(self, x, n_evals, converged):
        self.x, self.n_evals, self.converged = x, n_evals, converged


class _FakeCma:
    """solution() / get_state() of a P-population ActiveCMAES, values derived from p"""

    def __init__(self, n, lam):
        self.n, self.lam = n, lam

    def solution(self, p):
        return _Solution(np.arange(self.n) + 1000. * p, 7 * p, p % 2 == 1)

    def get_state(self, key, p):
        return {"xmean": np.full(self.n, p + 0.5), "sigma": np.array([0.25 * p]),
                "fitness": np.arange(self.lam) - float(p)}[key]


def test_dump_writes_every_population_as_float64(tmp_path):
    import bench
    wl = dict(bench.WORKLOADS["M"], n=6, np=10)
    bench.dump_outputs(_FakeCma(6, 10), wl, 5, str(tmp_path))
    out = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert set(out) == {"solution_x", "solution_n_evals", "solution_converged", "xmean", "sigma",
                        "fitness", "populations"}
    assert all(a.dtype == np.float64 for a in out.values())
    assert out["solution_x"].shape == (5, 6) and out["fitness"].shape == (5, 10)
    assert out["populations"].tolist() == [0, 1, 2, 3, 4]
    assert out["solution_x"][3, 2] == 3002. and out["solution_n_evals"].tolist() == [0, 7, 14, 21, 28]
    assert out["solution_converged"].tolist() == [0, 1, 0, 1, 0]
    assert out["sigma"].shape == (5,) and out["sigma"][4] == 1.0


def test_dump_samples_populations_beyond_the_limit(tmp_path, monkeypatch):
    import bench
    wl = dict(bench.WORKLOADS["M"], n=6, np=10)
    per_pop = 8 * (6 + 1 + 1 + 6 + 1 + 10)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 3 * per_pop)
    bench.dump_outputs(_FakeCma(6, 10), wl, 40, str(tmp_path / "a"))
    bench.dump_outputs(_FakeCma(6, 10), wl, 40, str(tmp_path / "b"))
    pops = np.load(tmp_path / "a" / "populations.npy")
    assert len(pops) == 3 and list(pops) == sorted(pops)
    assert np.array_equal(pops, np.load(tmp_path / "b" / "populations.npy"))   # fixed sample
    x = np.load(tmp_path / "a" / "solution_x.npy")
    assert np.array_equal(x[:, 0], 1000. * pops)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 3 * per_pop + 7 * 256          # + one .npy header per file


def test_help_lists_full_and_dump_outputs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "--full" in out.stdout and "--dump-outputs" in out.stdout
