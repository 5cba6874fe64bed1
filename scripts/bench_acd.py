#!/usr/bin/env python3
"""ACD throughput on one GPU: us per coordinate step of the whole handle and evaluations per second at
n = 128 on [-5, 5]^n, Rosenbrock and schwefel12, for 1, 256 and 4096 populations.

    python scripts/bench_acd.py [--sweeps 8] [--warmup 4] [--passes 5] [--pops 1,256,4096]

A coordinate step is two evaluations.  bbo_run advances one sweep (n steps) per poll: acd_sweep, and behind
a sweep that improved acd_ae, the decomposition and acd_post.  The rows report the five passes' median
with their least and largest, and from the engine's kernel timers (a separate pass with "profile" on) the
share of a sweep's device time spent in the update (acd_ae + acd_post) and in the decomposition.  The
speculative sweep was measured with this script and dropped (DESIGN.md section 3.16 has both timings), so
there is no `speculate` leg.  The reference's us per coordinate step on
one host core comes from scripts/gen_acd_golden.py --time.  One JSON line per measurement; nothing is
asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))      # the package, when run as scripts/bench_acd.py

N = 128


def measure(obj, P, sweeps, warmup, passes):
    import bboptpy_amd as bb
    lo, up = -5. * np.ones(N), 5. * np.ones(N)
    g = bb.ACD(2 ** 31 - 1, 0., 0., seed=1, populations=P)
    g.initialize(getattr(bb.objectives, obj), lo, up, np.zeros(P * N))
    g.run(warmup * N)
    steps = sweeps * N
    dts = []
    for _ in range(passes):
        t0 = time.perf_counter()
        g.run(steps)
        dts.append(time.perf_counter() - t0)
    itae0 = int(g.get_state("itae")[0])
    g.set_state("profile", [1.])
    g.run(steps)
    prof = g.get_state("profile").reshape(-1, 2)      # sweep, eval, ae, eigen, post: [ms, launches]
    g.set_state("profile", [0.])
    total = float(prof[:, 0].sum())
    dt = float(np.median(dts))
    return {"objective": obj, "P": P, "n": N, "sweeps": sweeps, "warmup_sweeps": warmup, "passes": passes,
            "us_per_step": 1e6 * dt / steps,
            "us_per_step_min_max": [1e6 * min(dts) / steps, 1e6 * max(dts) / steps],
            "evals_per_s": 2. * P * steps / dt,
            "updates_in_profiled_pass": int(g.get_state("itae")[0]) - itae0,
            "sweep_kernel_us_per_step": 1e3 * float(prof[0, 0]) / steps,
            "update_share": float(prof[2, 0] + prof[4, 0]) / total,
            "decomposition_share": float(prof[3, 0]) / total,
            "flags": sorted({int(g.get_state("flag", p)[0]) for p in range(0, P, max(1, P // 64))})}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--pops", default="1,256,4096")
    a = ap.parse_args()
    for obj in ("rosenbrock", "schwefel12"):
        for P in (int(v) for v in a.pops.split(",")):
            print(json.dumps(measure(obj, P, a.sweeps, a.warmup, a.passes)), flush=True)


if __name__ == "__main__":
    main()
