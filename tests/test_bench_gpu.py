"""GPU: a plain bench.py run does the headline alone -- set up, warm up, exactly --steps timed
generations, the result line -- and --dump-outputs writes what the last timed generation left,
the same for two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain(outdir):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                          "--populations", "4", "--steps", "7", "--warmup", "2",
                          "--dump-outputs", str(outdir)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_plain_run_times_the_steps_and_dumps_the_last_one(hip, tmp_path):
    rec = _plain(tmp_path / "a")
    assert rec["metric"] == "candidate-evals/sec" and rec["unit"] == "candidate-evals/s"
    assert rec["higher_is_better"] is True and rec["dtype"] == "f64"
    assert rec["steps"] == 7 and rec["warmup"] == 2 and rec["ms_per_step"] > 0
    # evaluations of 4 populations of lambda = 4096 over the 7 timed generations
    assert rec["value"] == pytest.approx(4 * 4096 * 7 / (7 * rec["ms_per_step"] * 1e-3))
    for leg in ("roofline", "single_population", "generations_to_tol", "bipop_scaling", "configs",
                "cpu_baseline"):
        assert rec[leg] is None, leg                    # --full only
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert all(v.dtype == np.float64 for v in a.values())
    assert a["solution_x"].shape == (4, 128) and a["fitness"].shape == (4, 4096)
    assert a["xmean"].shape == (4, 128) and a["sigma"].shape == (4,)
    # at least the (2 + 7) generations of 4096, the same in every population
    assert len(set(a["solution_n_evals"].tolist())) == 1 and a["solution_n_evals"][0] >= 9 * 4096
    assert np.isfinite(a["fitness"]).all() and (a["sigma"] > 0).all()
    _plain(tmp_path / "b")
    for name, v in a.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / (name + ".npy"))), name
