#!/usr/bin/env python3
"""SpiralSearch throughput on one GPU: ms per generation, evaluations per second and the time per
kernel at n = 128 on Rosenbrock, for np = 20 x 4096 populations, np = 4096 x 256 populations, and
one population of each.

    python scripts/bench_spiral.py [--steps 30] [--warmup 5] [--repeats 3]

Per shape, after the warm-up generations: `repeats` unprofiled passes (wall clock around run(),
which ends with a stream synchronisation; the median and the spread are reported) and one pass with
the engine's `profile` switch (an event pair around every launch on the engine's own stream: time
per kernel).  For spiral_rotate the share of the vector fp64 issue rate is its n (n - 1) / 2
rotations per point at 6 non-fused fp64 operations each over the kernel's time, against 256 CUs x
4 SIMDs x 16 fp64 lanes per clock x 2.4 GHz = 39.3e12 operations per second (half the 78.6 TFLOPS
the data sheet counts with fused multiply-adds).  The sweep repeats the profiled pass on the two
batched shapes with K = 1, 2, 4 and 8 fused stages and with the tile in global memory.  The
reference's ms per generation on one host core comes from scripts/gen_spiral_golden.py --time.
One JSON line per measurement; nothing is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

SLOTS = ("spiral_draw", "spiral_rotate", "spiral_eval", "spiral_best")
FP64_OPS_PER_S = 256 * 4 * 16 * 2.4e9
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))      # the package, when run as scripts/bench_spiral.py


def start(P, n, np_, steps):
    import bboptpy_amd as bb
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    g = bb.SpiralSearch(2 ** 31 - 1, 0., np_, seed=1, populations=P, poll_every=steps)
    g.initialize(bb.objectives.rosenbrock, lo, up, np.zeros(P * n))
    return g


def profiled(g, P, n, np_, steps):
    g.set_state("profile", [1.])
    g.run(steps)
    prof = g.get_state("profile").reshape(-1, 2)
    g.set_state("profile", [0.])
    per = {name: 1e3 * prof[i, 0] / max(prof[i, 1], 1.) for i, name in enumerate(SLOTS)}   # us per launch
    ops = 6. * P * np_ * n * (n - 1) / 2
    return per, ops / (per["spiral_rotate"] * 1e-6) / FP64_OPS_PER_S


def measure(P, n, np_, steps, warmup, repeats):
    g = start(P, n, np_, steps)
    g.run(warmup)
    dts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        g.run(steps)
        dts.append(time.perf_counter() - t0)
    dt = float(np.median(dts))
    per, share = profiled(g, P, n, np_, steps)
    return {"P": P, "n": n, "np": np_, "objective": "rosenbrock", "steps": steps, "rot_k": int(g.get_state("rot_k")[0]),
            "rot_split": int(g.get_state("rot_split")[0]),
            "evals_per_s": P * np_ * steps / dt, "ms_per_generation": 1e3 * dt / steps,
            "ms_per_generation_min_max": [1e3 * min(dts) / steps, 1e3 * max(dts) / steps],
            "kernel_us": per, "rotate_share_of_fp64_issue": share, "dominant": max(per, key=per.get)}


def sweep(P, n, np_, steps, warmup):
    out = []
    for k, dbg in ((1, 0), (2, 0), (4, 0), (8, 0), (8, 1)):
        g = start(P, n, np_, steps)
        g.set_state("rot_k", [float(k)])
        g.set_state("dbg", [float(dbg)])
        g.run(warmup)
        per, share = profiled(g, P, n, np_, steps)
        out.append({"sweep": True, "P": P, "n": n, "np": np_, "rot_k": k, "tile": "global" if dbg else "split at %d" % int(g.get_state("rot_split")[0]),
                    "rotate_us": per["spiral_rotate"], "rotate_share_of_fp64_issue": share})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    for P, np_ in ((4096, 20), (256, 4096), (1, 20), (1, 4096)):
        print(json.dumps(measure(P, 128, np_, a.steps, a.warmup, a.repeats)), flush=True)
    for P, np_ in ((4096, 20), (256, 4096)):
        for rec in sweep(P, 128, np_, a.steps, a.warmup):
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
