#!/usr/bin/env python3
"""AMALGAM throughput on one GPU: ms per generation of the whole handle and evaluations per second on
Rosenbrock at n = 128 -- iAMaLGaM (np = 113; populations = 1, 256, 4096) and AMaLGaM (np = 4361;
populations = 1, 256) -- in the inner mode (noparam=False).

    python scripts/bench_amalgam.py [--generations 100] [--warmup 10] [--repeats 5] [--quick]

Per measurement, after the warm-up generations: `repeats` passes of run(generations), wall clock
around run(), which ends every chunk with a stream synchronisation and a poll of the stop flags;
the median and the spread are reported.  Then one pass with the engine's `profile` switch (an event
pair around every launch): the per-kernel split without the host's share, and from it the share of
the fp64 matrix peak (78.6 TFLOP/s) the moments (ss n^2 flops per population: two per multiply-add
over the lower tiles) and the sampler (np n^2: the lower triangle of chol) reach, and the
factorisation's time.
The reference's ms per generation on one host core comes from scripts/gen_amalgam_golden.py --time.
One JSON line per measurement; nothing is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))      # the package, when run as scripts/bench_amalgam.py

KERNELS = ("amalgam_moments", "amalgam_factor", "amalgam_draw", "amalgam_points", "amalgam_eval", "amalgam_adapt",
           "amalgam_rank")
# (n, iamalgam, populations)
SHAPES = [(128, True, 1), (128, True, 256), (128, True, 4096), (128, False, 1), (128, False, 256)]
FP64_PEAK = 78.6e12


def measure(n, iam, P, generations, warmup, repeats):
    import bboptpy_amd as bb
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    g = bb.AMALGAM(2 ** 31 - 1, 0., 0., 0, iam, False, False, seed=1, populations=P, poll_every=generations)
    g.initialize(bb.objectives.rosenbrock, lo, up, np.zeros(P * n))
    np_, ss = int(g.get_state("np")[0]), int(g.get_state("ss")[0])
    g.run(warmup)
    dts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        done = g.run(generations)
        dts.append((time.perf_counter() - t0) / max(done, 1))
    dt = float(np.median(dts))
    g.set_state("profile", [1.])
    done = g.run(generations)
    prof = g.get_state("profile").reshape(-1, 2)
    g.set_state("profile", [0.])
    split = {k: float(prof[i, 0]) / max(done, 1) for i, k in enumerate(KERNELS)}
    return {"n": n, "mode": "iAMaLGaM" if iam else "AMaLGaM", "np": np_, "ss": ss, "P": P, "objective": "rosenbrock",
            "generations": generations, "ms_per_generation": 1e3 * dt, "spread": float((max(dts) - min(dts)) / dt),
            "evals_per_s": P * (np_ - 1) / dt, "kernel_ms_per_generation": split,
            "moments_share_of_fp64_matrix_peak": ss * n * n * P / (split["amalgam_moments"] * 1e-3) / FP64_PEAK,
            "sampler_share_of_fp64_matrix_peak": np_ * n * n * P / (split["amalgam_points"] * 1e-3) / FP64_PEAK,
            "factor_ms": split["amalgam_factor"], "route": g.get_state("route").astype(int).tolist(),
            "fact_fail": int(g.get_state("fact_fail")[0]), "stopped": int(g.get_state("stop")[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--generations", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="few generations, one population only")
    a = ap.parse_args()
    shapes = [s for s in SHAPES if s[2] == 1] if a.quick else SHAPES
    for n, iam, P in shapes:
        big = P * (113 if iam else 4361) > 2 ** 17
        gens = max(a.generations // 10, 8) if big else a.generations
        if a.quick:
            gens = 16
        print(json.dumps(measure(n, iam, P, gens, a.warmup if not a.quick else 8, a.repeats)), flush=True)


if __name__ == "__main__":
    main()
