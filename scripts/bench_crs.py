#!/usr/bin/env python3
"""CRS throughput on one GPU: us per evaluation of the whole handle and evaluations per second at
n = 128, np = 1290 (Price's 10 (n + 1)), Rosenbrock on [-5, 5]^n, for 1, 256 and 4096 populations.

    python scripts/bench_crs.py [--iterations 1024] [--warmup 1024] [--repeats 3] [--quick]

  fused        bbo_run in chunks of 256 iterations: crs_steps walks whole iterations per launch and a
               launch ends for a population after 8 steps per iteration of the chunk at the latest
  step by step "launch_evals" = 1: every launch ends after ONE drawn trial or ONE evaluation and the
               next resumes the walk (what the launch bound costs at its smallest setting)
  repair       the loop of the paper (repair=True), fused

An iteration costs as many trials and evaluations as the walk takes, so the unit is the evaluation: the
rows report the evaluations and the drawn trials per iteration next to the times.  The pool starts
uniform in the box; a trial of 128 coordinates leaves it far more often than it stays inside, so the
early iterations are deep recursions ("maxdepth") and the cost per iteration falls as the pool
contracts: the warm-up and the measured span are stated in iterations.  The reference's us per iteration
and evaluation on one host core comes from scripts/gen_crs_golden.py --time.  One JSON line per
measurement; nothing is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))      # the package, when run as scripts/bench_crs.py

N, NP = 128, 1290


def start(P, launch_evals=0, repair=False):
    import bboptpy_amd as bb
    lo, up = -5. * np.ones(N), 5. * np.ones(N)
    g = bb.CRS(2 ** 31 - 1, NP, 0., seed=1, populations=P, repair=repair)
    g.initialize(bb.objectives.rosenbrock, lo, up, np.zeros(P * N))
    g.set_state("launch_evals", [float(launch_evals)])
    return g


def counters(g, P):
    ps = range(0, P, max(1, P // 64))
    return {k: float(np.mean([g.get_state(k, p)[0] for p in ps])) for k in ("fev", "trials", "it", "stale")}


def measure(what, P, iterations, warmup, repeats, launch_evals=0, repair=False):
    g = start(P, 0, repair)
    g.run(warmup)           # (fused whatever is measured: the same bits, and the pool in the same state)
    g.set_state("launch_evals", [float(launch_evals)])
    dts, evs, trs = [], [], []
    deepest = 0
    for _ in range(repeats):
        c0 = counters(g, P)
        t0 = time.perf_counter()
        g.run(iterations)
        dts.append(time.perf_counter() - t0)
        c1 = counters(g, P)
        evs.append(c1["fev"] - c0["fev"])
        trs.append(c1["trials"] - c0["trials"])
        deepest = max(deepest, int(g.get_state("maxdepth")[0]))
    k = int(np.argsort(dts)[len(dts) // 2])     # the median span, with its own counts
    dt, ev, tr = dts[k], evs[k], trs[k]
    g.set_state("profile", [1.])
    c0 = counters(g, P)
    g.run(iterations)
    c1 = counters(g, P)
    prof = g.get_state("profile").reshape(-1, 2)
    g.set_state("profile", [0.])
    flags = sorted({int(g.get_state("flag", p)[0]) for p in range(0, P, max(1, P // 64))})
    return {"what": what, "P": P, "n": N, "np": NP, "objective": "rosenbrock", "iterations": iterations,
            "warmup": warmup, "chunk": int(g.get_state("chunk")[0]), "wg": int(g.get_state("wg")[0]),
            "launch_evals": launch_evals, "repair": int(repair),
            "evaluations_per_iteration": ev / iterations, "trials_per_iteration": tr / iterations,
            "us_per_iteration": 1e6 * dt / iterations,
            "us_per_evaluation": 1e6 * dt / ev,
            "us_per_evaluation_min_max": [1e6 * min(d / e for d, e in zip(dts, evs)),
                                          1e6 * max(d / e for d, e in zip(dts, evs))],
            "evals_per_s": P * ev / dt,
            "steps_kernel_us_per_evaluation": 1e3 * float(prof[2, 0]) / (c1["fev"] - c0["fev"]),
            "steps_kernel_launches": int(prof[2, 1]),
            "stale_share": c1["stale"] / c1["it"], "maxdepth_seen": deepest, "flags": flags}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="fused only")
    a = ap.parse_args()
    pops = (1, 256, 4096)
    for P in pops:
        print(json.dumps(measure("fused", P, a.iterations, a.warmup, a.repeats)), flush=True)
    if a.quick:
        return
    for P in pops:
        print(json.dumps(measure("step by step", P, max(a.iterations // 16, 32), a.warmup, a.repeats, launch_evals=1)),
              flush=True)
    for P in pops:
        print(json.dumps(measure("repair", P, a.iterations, a.warmup, a.repeats, repair=True)), flush=True)


if __name__ == "__main__":
    main()
