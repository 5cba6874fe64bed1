#!/usr/bin/env python3
"""SSDE throughput on one GPU: ms per generation of the whole handle and evaluations per second at
n = 128, npinit = 100 on Rosenbrock, usede off and on (with usede a member whose spherical trial loses
evaluates a DE trial too, so the evaluations are counted from the handles' own fev).

    python scripts/bench_ssde.py [--generations 100] [--warmup 20] [--repeats 5] [--quick]

npmin = npinit keeps the pool at 100 members and the budget is out of reach, so every generation does the
same work (R = fev / mfev stays near 0: with usede the "explore" strategy).  Per measurement, after the
warm-up generations: `repeats` passes of run(generations), wall clock around run(), which ends every chunk
with a stream synchronisation and a poll of the stop flags; the median and the spread are reported.  What is
measured:
  fused   populations = 1, 256, 4096: one launch per generation
  phase   populations = 1: the generation one evaluation at a time through bbo_ssde_phase (what a host
          objective pays in launches, without the objective's own time; fewer generations)
and one pass with the engine's `profile` switch (an event pair around the launch: the kernel's own time
without the host's share).  The reference's ms per generation on one host core comes from
scripts/gen_ssde_golden.py --time.  One JSON line per measurement; nothing is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))      # the package, when run as scripts/bench_ssde.py

N, NP = 128, 100


def start(P, usede, n=N):
    import bboptpy_amd as bb
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    g = bb.SSDE(2 ** 31 - 1, NP, 0., patience=2 ** 30, npmin=NP, usede=usede, seed=1, populations=P)
    g.initialize(bb.objectives.rosenbrock, lo, up, np.zeros(P * n))
    return g


def fev_of(g, P):
    return sum(int(g.get_state("fev", p)[0]) for p in range(min(P, 32))) / float(min(P, 32))


def measure(P, usede, generations, warmup, repeats, n=N):
    g = start(P, usede, n)
    g.run(warmup)
    fev0 = fev_of(g, P)
    dts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        g.run(generations)
        dts.append(time.perf_counter() - t0)
    evals = (fev_of(g, P) - fev0) / (repeats * generations)     # per generation and population
    dt = float(np.median(dts))
    g.set_state("profile", [1.])
    g.run(generations)
    prof = g.get_state("profile").reshape(-1, 2)
    g.set_state("profile", [0.])
    return {"what": "fused", "P": P, "n": n, "npinit": NP, "usede": int(usede), "objective": "rosenbrock",
            "generations": generations, "wg": int(g.get_state("wg")[0]),
            "ms_per_generation": 1e3 * dt / generations,
            "ms_per_generation_min_max": [1e3 * min(dts) / generations, 1e3 * max(dts) / generations],
            "evals_per_generation": evals, "evals_per_s": P * evals * generations / dt,
            "kernel_ms_per_generation": float(prof[1, 0]) / generations}


def measure_phase(P, usede, generations, warmup, repeats):
    g = start(P, usede)
    g.run(warmup)
    dts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(generations):
            while g.phase(0):
                g.phase(1)
                g.phase(2)
        dts.append(time.perf_counter() - t0)
    dt = float(np.median(dts))
    return {"what": "phase", "P": P, "n": N, "npinit": NP, "usede": int(usede), "generations": generations,
            "ms_per_generation": 1e3 * dt / generations,
            "ms_per_generation_min_max": [1e3 * min(dts) / generations, 1e3 * max(dts) / generations]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--generations", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="populations = 256 only, no phase path")
    a = ap.parse_args()
    pops = (256,) if a.quick else (1, 256, 4096)
    for usede in (False, True):
        for P in pops:
            print(json.dumps(measure(P, usede, a.generations, a.warmup, a.repeats)), flush=True)
    if a.quick:
        return
    print(json.dumps(measure_phase(1, False, max(a.generations // 20, 3), 3, 3)), flush=True)


if __name__ == "__main__":
    main()
