#!/usr/bin/env python3
"""xNES throughput on one GPU: ms per generation of the whole handle and evaluations per second on
Rosenbrock at n = 128 (np = 18; populations = 1, 256, 4096) and n = 512 (np = 22; populations = 1,
256).

    python scripts/bench_xnes.py [--generations 200] [--warmup 20] [--repeats 5] [--quick]

Per measurement, after the warm-up generations: `repeats` passes of run(generations), wall clock
around run(), which ends every chunk with a stream synchronisation and a poll of the stop flags;
the median and the spread are reported.  Then one pass with the engine's `profile` switch (an event
pair around every launch): the per-kernel split without the host's share, and from it the share of
the HBM peak the two passes over B reach (xnes_points reads B, xnes_adapt reads and writes it:
3 n^2 doubles per population and generation; 8 TB/s).  The reference's ms per generation on one host
core comes from scripts/gen_xnes_golden.py --time.  One JSON line per measurement; nothing is
asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))      # the package, when run as scripts/bench_xnes.py

KERNELS = ("xnes_draw", "xnes_points", "xnes_rank", "xnes_step", "xnes_adapt")
SHAPES = [(128, 1), (128, 256), (128, 4096), (512, 1), (512, 256)]
HBM_PEAK = 8.0e12


def measure(n, P, generations, warmup, repeats):
    import bboptpy_amd as bb
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    g = bb.xNES(2 ** 31 - 1, 0., seed=1, populations=P, poll_every=generations)
    g.initialize(bb.objectives.rosenbrock, lo, up, np.zeros(P * n))
    np_ = int(g.get_state("np")[0])
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
    passes_ms = split["xnes_points"] + split["xnes_adapt"]
    return {"n": n, "np": np_, "P": P, "objective": "rosenbrock", "generations": generations,
            "ms_per_generation": 1e3 * dt, "spread": float((max(dts) - min(dts)) / dt),
            "evals_per_s": P * np_ / dt, "kernel_ms_per_generation": split,
            "hbm_share_of_the_passes_over_B": 3. * 8. * n * n * P / (passes_ms * 1e-3) / HBM_PEAK,
            "route": int(g.get_state("route")[0]), "fact_fail": int(g.get_state("fact_fail")[0]),
            "stopped": int(g.get_state("stop")[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--generations", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="few generations, the small shapes only")
    a = ap.parse_args()
    shapes = SHAPES[:2] if a.quick else SHAPES
    for n, P in shapes:
        gens = a.generations if P * n * n < 2 ** 24 else max(a.generations // 10, 8)
        if a.quick:
            gens = 16
        print(json.dumps(measure(n, P, gens, a.warmup if not a.quick else 8, a.repeats)), flush=True)


if __name__ == "__main__":
    main()
