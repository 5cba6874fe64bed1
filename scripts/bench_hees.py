#!/usr/bin/env python3
"""HEES throughput on one GPU: ms per generation, evaluations per second and the time per kernel at
n = 128 on Rosenbrock, for np = 0 (mu = 9) x 4096 populations, np = 2048 x 256 populations, and one
population of each.

    python scripts/bench_hees.py [--steps 30] [--warmup 5]

Two passes per shape after the warm-up generations: one unprofiled (wall clock around run(), which
ends with a stream synchronisation) and one with the engine's `profile` switch (an event pair
around every launch on the engine's own stream: time per kernel, and which of draw, ortho, points
and update + adapt dominates).  The reference's ms per generation on one host core comes from
scripts/gen_hees_golden.py --time.  One JSON line per measurement; nothing is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

SLOTS = ("hees_draw", "hees_ortho", "hees_points", "hees_rank", "hees_update", "hees_adapt", "hees_finish")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))      # the package, when run as scripts/bench_hees.py


def measure(P, n, np_, steps, warmup):
    import bboptpy_amd as bb
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    g = bb.HEES(2 ** 31 - 1, 0., np=np_, seed=1, populations=P, poll_every=steps)
    g.initialize(bb.objectives.rosenbrock, lo, up, 3. * np.ones((P, n)))
    mu = int(g.get_state("mu")[0])
    g.run(warmup)
    t0 = time.perf_counter()
    g.run(steps)
    dt = time.perf_counter() - t0
    g.set_state("profile", [1.])
    g.run(steps)
    prof = g.get_state("profile").reshape(-1, 2)
    per = {name: 1e3 * prof[i, 0] / max(prof[i, 1], 1.) for i, name in enumerate(SLOTS)}   # us per launch
    return {"P": P, "n": n, "np": np_, "mu": mu, "objective": "rosenbrock", "steps": steps,
            "evals_per_s": P * (2 * mu + 1) * steps / dt, "ms_per_generation": 1e3 * dt / steps,
            "kernel_us": per, "dominant": max(per, key=per.get)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    for P, np_ in ((4096, 0), (256, 2048), (1, 0), (1, 2048)):
        print(json.dumps(measure(P, 128, np_, a.steps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
