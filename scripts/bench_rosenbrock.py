#!/usr/bin/env python3
"""Rosenbrock (the rotating-axes search) throughput on one GPU: us per line search of the whole handle and
evaluations per second on the Rosenbrock objective over [-5, 5]^n at n = 32 and 128, for 1, 256 and 4096
populations (independent searches from different starts), in both forms of the walk: wide (a wavefront per point
of a batch, 256 threads) and narrow (one wavefront, the points in turn).

    python scripts/bench_rosenbrock.py [--steps 512] [--warmup 128] [--passes 5] [--pops 1,256,4096] [--ns 32,128]

A step is one iterate() of the reference: a line search of about eight evaluations and its bookkeeping; every
n + 1 searches or so the n^2 sums of Palmer's orthogonalisation.  "orth_share" is the orthogonalisations' share of
the time inside rosen_walk over the timed passes, from the kernel's own constant-rate clock ("orth_ticks" over
"walk_ticks", summed over the probed populations), which is their share of a stage where every stage ends in one;
"orths_per_population" counts them.  bbo_run advances 64 searches per launch and poll.  The rows report the
five passes' median with their least and largest; the evaluations are the handle's own count over the timed
passes.  The reference's us per line search on one host core comes from scripts/gen_rosenbrock_golden.py --time.
One JSON line per measurement; nothing is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))      # the package, when run as scripts/bench_rosenbrock.py


def measure(n, P, wide, steps, warmup, passes):
    import bboptpy_amd as bb
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    guess = np.random.default_rng(n).uniform(-3., 3., P * n)
    g = bb.Rosenbrock(2 ** 31 - 1, 0., 1., seed=1, populations=P, wide=wide)
    g.initialize(bb.objectives.rosenbrock, lo, up, guess)
    g.run(warmup)
    probe = range(0, P, max(1, P // 64))
    fev0 = [int(g.get_state("fev", p)[0]) for p in probe]
    orth0 = [int(g.get_state("orths", p)[0]) for p in probe]
    ticks0 = [[float(g.get_state(k, p)[0]) for p in probe] for k in ("orth_ticks", "walk_ticks")]
    dts = []
    for _ in range(passes):
        t0 = time.perf_counter()
        g.run(steps)
        dts.append(time.perf_counter() - t0)
    fev1 = [int(g.get_state("fev", p)[0]) for p in probe]
    orth1 = [int(g.get_state("orths", p)[0]) for p in probe]
    ticks1 = [[float(g.get_state(k, p)[0]) for p in probe] for k in ("orth_ticks", "walk_ticks")]
    share = float(np.sum(np.subtract(ticks1[0], ticks0[0])) / np.sum(np.subtract(ticks1[1], ticks0[1])))
    per_step = float(np.mean(np.subtract(fev1, fev0))) / (passes * steps)
    dt = float(np.median(dts))
    return {"n": n, "P": P, "wide": int(wide), "steps": steps, "warmup_steps": warmup, "passes": passes,
            "us_per_search": 1e6 * dt / steps,
            "us_per_search_min_max": [1e6 * min(dts) / steps, 1e6 * max(dts) / steps],
            "evals_per_search": per_step, "evals_per_s": per_step * P * steps / dt,
            "orth_share": share, "orths_per_population": float(np.mean(np.subtract(orth1, orth0))),
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
            for wide in (True, False):
                print(json.dumps(measure(n, P, wide, a.steps, a.warmup, a.passes)), flush=True)


if __name__ == "__main__":
    main()
