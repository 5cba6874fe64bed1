#!/usr/bin/env python3
"""NSHS throughput on one GPU: us per iteration of the whole handle and evaluations per second at
n = 128, hms = 20 on Rosenbrock (one iteration is one evaluation per population).

    python scripts/bench_nshs.py [--iterations 4096] [--warmup 512] [--repeats 5] [--quick]

Per measurement, after the warm-up iterations: `repeats` passes of run(iterations), wall clock
around run(), which ends every chunk with a stream synchronisation and a poll of the stop flags;
the median and the spread are reported.  What is measured:
  fused        populations = 1, 256, 4096, 16384 with the default chunk (iterations per launch)
  one by one   the same with poll_every = 1: one iteration per launch, what the fusion buys
               (fewer iterations: every one is a launch, a synchronisation and a poll)
  global       the same with dbg = 1: the harmony memory gathered from global memory whatever its
               size (at hms = 20 it exceeds the LDS budget, so these repeat the fused rows)
  chunk        64, 256 and 1024 iterations per launch at populations = 4096
  workgroup    64, 128 and 256 threads at populations = 4096
  hms 6        a memory that fits the LDS budget, in LDS and gathered from global memory
and one pass with the engine's `profile` switch (an event pair around the launch: the kernel's own
time without the host's share).  The reference's us per iteration on one host core comes from
scripts/gen_nshs_golden.py --time.  One JSON line per measurement; nothing is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))      # the package, when run as scripts/bench_nshs.py

N, HMS = 128, 20


def start(P, poll=None, dbg=0, wg=0, hms=HMS):
    import bboptpy_amd as bb
    lo, up = -5. * np.ones(N), 5. * np.ones(N)
    kw = {} if poll is None else {"poll_every": poll}
    g = bb.NSHS(2 ** 31 - 1, hms, seed=1, populations=P, **kw)
    g.initialize(bb.objectives.rosenbrock, lo, up, np.zeros(P * N))
    g.set_state("dbg", [float(dbg)])
    g.set_state("wg", [float(wg)])
    return g


def measure(what, P, iterations, warmup, repeats, poll=None, dbg=0, wg=0, hms=HMS):
    g = start(P, poll, dbg, wg, hms)
    g.run(warmup)
    dts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        g.run(iterations)
        dts.append(time.perf_counter() - t0)
    dt = float(np.median(dts))
    g.set_state("profile", [1.])
    g.run(iterations)
    prof = g.get_state("profile").reshape(-1, 2)
    g.set_state("profile", [0.])
    kernel_ms = float(prof[4, 0])      # the slot of nshs_steps
    return {"what": what, "P": P, "n": N, "hms": hms, "objective": "rosenbrock", "iterations": iterations,
            "chunk": int(g.get_state("chunk")[0]), "wg": int(g.get_state("wg")[0]),
            "hm_in_lds": int(g.get_state("hm_in_lds")[0]),
            "us_per_iteration": 1e6 * dt / iterations,
            "us_per_iteration_min_max": [1e6 * min(dts) / iterations, 1e6 * max(dts) / iterations],
            "evals_per_s": P * iterations / dt,
            "steps_kernel_us_per_iteration": 1e3 * kernel_ms / iterations,
            "acceptance": float(np.mean([g.get_state("accepted", p)[0] for p in range(min(P, 64))]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="populations = 4096 only, no sweeps")
    a = ap.parse_args()
    pops = (4096,) if a.quick else (1, 256, 4096, 16384)
    for P in pops:
        print(json.dumps(measure("fused", P, a.iterations, a.warmup, a.repeats)), flush=True)
    if a.quick:
        return
    for P in pops:
        print(json.dumps(measure("one by one", P, max(a.iterations // 16, 64), 32, a.repeats, poll=1)), flush=True)
    for P in pops:
        print(json.dumps(measure("global", P, a.iterations, a.warmup, a.repeats, dbg=1)), flush=True)
    for chunk in (64, 256, 1024):
        print(json.dumps(measure("chunk", 4096, a.iterations, a.warmup, a.repeats, poll=chunk)), flush=True)
    for wg in (64, 128, 256):
        print(json.dumps(measure("workgroup", 4096, a.iterations, a.warmup, a.repeats, wg=wg)), flush=True)
    for P in (256, 4096):           # a memory small enough for LDS, and the same gathered from global memory
        for dbg in (0, 1):
            print(json.dumps(measure("hms 6", P, a.iterations, a.warmup, a.repeats, dbg=dbg, hms=6)), flush=True)


if __name__ == "__main__":
    main()
