#!/usr/bin/env python3
"""SLPSO throughput on one GPU: ms per generation of the whole handle and evaluations per second at
n = 128, np = 20 on Rosenbrock (one generation is np particle steps plus the Algorithm 2 evaluations
the improving moves start, so the evaluations are counted from the handles' own fev).

    python scripts/bench_slpso.py [--generations 200] [--warmup 50] [--repeats 5] [--quick]

Per measurement, after the warm-up generations: `repeats` passes of run(generations), wall clock around
run(), which ends every chunk with a stream synchronisation and a poll of the stop flags; the median
and the spread are reported.  What is measured:
  speculative  populations = 1, 256, 4096: Algorithm 2 with a trial per wavefront (the default at n > 64)
  sequential   the same with dbg = 1: Algorithm 2 one trial at a time
  phase        populations = 1: the generation one evaluation at a time through bbo_slpso_phase (what a
               host objective pays in launches, without the objective's own time; fewer generations)
and one pass with the engine's `profile` switch (an event pair around the launch: the kernel's own time
without the host's share).  The same seed runs under both forms of Algorithm 2, which are bit-identical
(tests/test_slpso_gpu.py), so both rows do the same work.  The reference's ms per generation on one host
core comes from scripts/gen_slpso_golden.py --time.  One JSON line per measurement; nothing is
asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))      # the package, when run as scripts/bench_slpso.py

N, NP = 128, 20


def start(P, dbg=0, n=N):
    import bboptpy_amd as bb
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    g = bb.SLPSO(2 ** 31 - 1, 0., NP, seed=1, populations=P)
    g.initialize(bb.objectives.rosenbrock, lo, up, np.zeros(P * n))
    g.set_state("dbg", [float(dbg)])
    return g


def fev_of(g, P):
    return sum(int(g.get_state("fev", p)[0]) for p in range(min(P, 32))) / float(min(P, 32))


def measure(what, P, generations, warmup, repeats, dbg=0, n=N):
    g = start(P, dbg, n)
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
    return {"what": what, "P": P, "n": n, "np": NP, "objective": "rosenbrock", "generations": generations,
            "wg": int(g.get_state("wg")[0]), "speculative": int(g.get_state("speculative")[0]),
            "ms_per_generation": 1e3 * dt / generations,
            "ms_per_generation_min_max": [1e3 * min(dts) / generations, 1e3 * max(dts) / generations],
            "evals_per_generation": evals, "evals_per_s": P * evals * generations / dt,
            "kernel_ms_per_generation": float(prof[1, 0]) / generations}


def measure_phase(P, generations, warmup, repeats):
    g = start(P)
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
    return {"what": "phase", "P": P, "n": N, "np": NP, "generations": generations,
            "ms_per_generation": 1e3 * dt / generations,
            "ms_per_generation_min_max": [1e3 * min(dts) / generations, 1e3 * max(dts) / generations]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--generations", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="populations = 256 only, no phase path")
    a = ap.parse_args()
    pops = (256,) if a.quick else (1, 256, 4096)
    for P in pops:
        for what, dbg in (("speculative", 0), ("sequential", 1)):
            print(json.dumps(measure(what, P, a.generations, a.warmup, a.repeats, dbg=dbg)), flush=True)
    if a.quick:
        return
    for n in (64, 256):         # one wavefront (no speculative form) and four
        for what, dbg in (("speculative", 0), ("sequential", 1)):
            if n == 64 and dbg:
                continue
            print(json.dumps(measure(what, 256, a.generations, a.warmup, a.repeats, dbg=dbg, n=n)), flush=True)
    print(json.dumps(measure_phase(1, max(a.generations // 20, 5), 5, 3)), flush=True)


if __name__ == "__main__":
    main()
