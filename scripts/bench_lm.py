#!/usr/bin/env python3
"""LmCMAES throughput on one GPU: ms per generation of the whole handle and evaluations per second
on the ellipsoid at n = 1024, lambda = 24 (populations = 1, 256, 4096) and n = 4096, lambda = 28
(populations = 1, 256), default memory (m = 64 and 128), Rademacher sampling.

    python scripts/bench_lm.py [--generations 200] [--warmup 40] [--repeats 5] [--quick]

Per measurement, after the warm-up generations (which also fill a part of the memory: the cost of
a generation grows with the slots in use, so `memlen` is reported): `repeats` passes of
run(generations), wall clock around run(), which ends every chunk with a stream synchronisation and
a poll of the stop flags; the median and the spread are reported.  Then one pass with the engine's
`profile` switch (an event pair around every launch): the per-kernel split without the host's
share.  The reference's ms per generation on one host core comes from scripts/gen_lm_golden.py's
harness run for the same shape.  One JSON line per measurement; nothing is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))      # the package, when run as scripts/bench_lm.py

KERNELS = ("lm_draw", "lm_sample", "lm_eval", "lm_rank", "lm_update", "lm_history_stop")
SHAPES = [(1024, 24, 1), (1024, 24, 256), (1024, 24, 4096), (4096, 28, 1), (4096, 28, 256)]


def measure(n, lam, P, generations, warmup, repeats):
    import bboptpy_amd as bb
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    g = bb.LmCMAES(2 ** 31 - 1, 0., lam, seed=1, populations=P)
    g.initialize(bb.objectives.ellipsoid, lo, up, np.tile(3. * np.ones(n), P))
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
    return {"n": n, "lambda": lam, "P": P, "memory": int(g.get_state("memory")[0]),
            "memlen": int(g.get_state("memlen")[0]), "objective": "ellipsoid", "generations": generations,
            "ms_per_generation": 1e3 * dt, "spread": float((max(dts) - min(dts)) / dt),
            "evals_per_s": P * lam / dt, "kernel_ms_per_generation": split,
            "stopped": int(g.get_state("stop")[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--generations", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="few generations, the small shapes only")
    a = ap.parse_args()
    shapes = SHAPES[:2] if a.quick else SHAPES
    for n, lam, P in shapes:
        gens = a.generations if P * n < 2 ** 21 else max(a.generations // 10, 8)
        if a.quick:
            gens = 16
        print(json.dumps(measure(n, lam, P, gens, a.warmup if not a.quick else 8, a.repeats)), flush=True)


if __name__ == "__main__":
    main()
