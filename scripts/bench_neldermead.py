#!/usr/bin/env python3
"""NelderMead throughput on one GPU: us per simplex step of the whole handle and evaluations per second on
Rosenbrock over [-5, 5]^n at n = 32 and 128, for 1, 256 and 4096 populations (independent simplexes from
different starts), with the simplex of a launch in LDS and in HBM.

    python scripts/bench_neldermead.py [--steps 512] [--warmup 128] [--passes 5] [--pops 1,256,4096] [--ns 32,128]

A step is one iterate() of the reference: one or two evaluations, n + 3 where the simplex shrinks.  bbo_run
advances 64 steps per launch and poll.  The rows report the five passes' median with their least and largest;
the evaluations are the handle's own count over the timed passes.  The reference's us per step on one host core
comes from scripts/gen_neldermead_golden.py --time.  The speculative step was measured with this script and dropped (DESIGN.md section 3.19 has both
timings), so there is no `speculate` leg.  One JSON line per measurement; nothing is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))      # the package, when run as scripts/bench_neldermead.py


def measure(n, P, lds, steps, warmup, passes):
    import bboptpy_amd as bb
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    guess = np.random.default_rng(n).uniform(-3., 3., P * n)
    g = bb.NelderMead(2 ** 31 - 1, 0., 1., seed=1, populations=P, lds=lds)
    g.initialize(bb.objectives.rosenbrock, lo, up, guess)
    g.run(warmup)
    probe = range(0, P, max(1, P // 64))
    fev0 = [int(g.get_state("fev", p)[0]) for p in probe]
    dts = []
    for _ in range(passes):
        t0 = time.perf_counter()
        g.run(steps)
        dts.append(time.perf_counter() - t0)
    fev1 = [int(g.get_state("fev", p)[0]) for p in probe]
    per_step = float(np.mean(np.subtract(fev1, fev0))) / (passes * steps)
    dt = float(np.median(dts))
    return {"n": n, "P": P, "lds": int(lds), "steps": steps, "warmup_steps": warmup, "passes": passes,
            "us_per_step": 1e6 * dt / steps,
            "us_per_step_min_max": [1e6 * min(dts) / steps, 1e6 * max(dts) / steps],
            "evals_per_step": per_step, "evals_per_s": per_step * P * steps / dt,
            "flags": sorted({int(g.get_state("flag", p)[0]) for p in probe})}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=128)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--pops", default="1,256,4096")
    ap.add_argument("--ns", default="32,128")
    a = ap.parse_args()
    for n in (int(v) for v in a.ns.split(",")):
        for P in (int(v) for v in a.pops.split(",")):
            for lds in (True, False):
                print(json.dumps(measure(n, P, lds, a.steps, a.warmup, a.passes)), flush=True)


if __name__ == "__main__":
    main()
