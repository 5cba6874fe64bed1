#!/usr/bin/env python3
"""Mayfly throughput on one GPU: ms per generation of the whole handle and evaluations per second at n = 128
on Rosenbrock over [-5, 5]^n, np = 20 and np = 256, for 1, 256 and 4096 populations.

    python scripts/bench_mayfly.py [--passes 5] [--quick]

  generation   bbo_run: a generation is 3 np + nmut evaluations (np females, np males, np offspring, nmut
               mutated flies) in ten launches, the male loop as prefix-commit rounds of `window` males
  windows      the same with "window" = 1 (the sequential loop), 4 (the default: the wavefronts of the
               workgroup) and 0 (all remaining males), at one population and at 4096: the state is the same
               bit for bit, only the time and the share of male evaluations that are dropped differ

Each figure is the median of `passes` spans with the least and the largest next to it.  "dropped_share" is
the male evaluations formed ahead of their turn and discarded over the male evaluations that were kept.  The
reference's ms per generation on one host core comes from scripts/gen_mayfly_golden.py --time.  One JSON
line per measurement; nothing is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))      # the package, when run as scripts/bench_mayfly.py

N = 128


def start(P, np_, window):
    import bboptpy_amd as bb
    g = bb.Mayfly(np_, 2 ** 31 - 1, seed=1, populations=P)
    g.initialize(bb.objectives.rosenbrock, -5. * np.ones(N), 5. * np.ones(N), np.zeros(P * N))
    g.set_state("window", [float(window)])
    return g


def measure(what, P, np_, window, gens, warmup, passes):
    g = start(P, np_, window)
    g.run(warmup)
    ps = range(0, P, max(1, P // 64))
    count = lambda k: float(np.mean([g.get_state(k, p)[0] for p in ps]))
    d0, f0 = count("dropped"), count("fev")
    dts = []
    for _ in range(passes):
        t0 = time.perf_counter()
        g.run(gens)
        dts.append(time.perf_counter() - t0)
    dropped, fev = count("dropped") - d0, count("fev") - f0
    per = fev / (gens * passes)                 # evaluations per generation and population
    dt = float(np.median(dts))
    g.set_state("profile", [1.])
    g.run(gens)
    prof = g.get_state("profile").reshape(-1, 2)
    names = ("init", "begin", "females", "males", "rank", "cross", "mutate", "merge", "resolve", "copy")
    return {"what": what, "P": P, "n": N, "np": np_, "nmut": int(g.get_state("nmut")[0]), "window": window,
            "objective": "rosenbrock", "generations": gens, "warmup": warmup, "passes": passes,
            "evaluations_per_generation": per,
            "ms_per_generation": 1e3 * dt / gens,
            "ms_per_generation_min_max": [1e3 * min(dts) / gens, 1e3 * max(dts) / gens],
            "evals_per_s": P * per * gens / dt,
            "dropped_share": dropped / (np_ * gens * passes),
            "kernel_ms_per_generation": {k: float(prof[i, 0]) / gens for i, k in enumerate(names) if prof[i, 1] > 0}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="np = 256 only, no window comparison")
    a = ap.parse_args()
    for np_ in ((256,) if a.quick else (20, 256)):
        for P in (1, 256, 4096):
            gens = 64 if P * np_ <= 256 * 256 else 8
            print(json.dumps(measure("generation", P, np_, 4, gens, gens, a.passes)), flush=True)
    if a.quick:
        return
    for P in (1, 4096):
        for window in (1, 4, 0):
            gens = 64 if P == 1 else 8
            print(json.dumps(measure("windows", P, 256, window, gens, gens, a.passes)), flush=True)


if __name__ == "__main__":
    main()
