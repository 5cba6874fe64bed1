#!/usr/bin/env python3
"""JAYA throughput on one GPU: evaluations per second and the time per kernel at
n = 128, np = 4096, Rastrigin, for P = 256 populations of one handle and for P = 1.

    python scripts/bench_jaya.py [--steps 50] [--warmup 10]

Two passes per shape after the warm-up generations: one unprofiled (wall clock around run(), which
ends with a stream synchronisation: evaluations/s) and one with the engine's `profile` switch (an
event pair around every launch on the engine's own stream: time per kernel).  jaya_evolve's bytes
are counted as the 8 n bytes every member's row is read with -- a lower bound, the rows of accepted
trials are also written -- and set against the 8 TB/s HBM peak of the MI355X.  One JSON line per
shape."""
import argparse
import json
import time

import numpy as np

import bboptpy_amd as bb

HBM_PEAK = 8.0e12
SLOTS = ("jaya_partition", "jaya_evolve", "jaya_finish")


def measure(P, n, np_, steps, warmup):
    lo, up = -5.12 * np.ones(n), 5.12 * np.ones(n)
    g = bb.JAYA(2 ** 31 - 1, 0., np_, 8, seed=1, populations=P, poll_every=steps)
    g.initialize(bb.objectives.rastrigin, lo, up, np.zeros((P, n)))
    g.run(warmup)
    t0 = time.perf_counter()
    g.run(steps)
    dt = time.perf_counter() - t0
    g.set_state("profile", [1.])
    g.run(steps)
    prof = g.get_state("profile").reshape(-1, 2)
    per = {name: 1e3 * prof[i, 0] / max(prof[i, 1], 1.) for i, name in enumerate(SLOTS)}   # us per launch
    evolve_s = per["jaya_evolve"] * 1e-6
    return {"P": P, "n": n, "np": np_, "objective": "rastrigin", "steps": steps,
            "evals_per_s": P * np_ * steps / dt, "us_per_generation": 1e6 * dt / steps,
            "kernel_us": per,
            "evolve_read_bytes_per_s": P * np_ * n * 8 / evolve_s,
            "evolve_fraction_of_hbm_peak": P * np_ * n * 8 / evolve_s / HBM_PEAK}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    a = ap.parse_args()
    for P in (256, 1):
        print(json.dumps(measure(P, 128, 4096, a.steps, a.warmup)))


if __name__ == "__main__":
    main()
