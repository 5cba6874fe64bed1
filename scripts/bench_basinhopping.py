#!/usr/bin/env python3
"""BasinHopping throughput on one GPU: ms per hop of the whole handle and evaluations per second on the Rosenbrock
objective over [-5, 5]^n at n = 32 and 128, mit = 20, for 1, 256 and 4096 chains, over both device-resident
minimisers with the parameters of their own bench scripts' shapes and a budget of 1000 evaluations per minimisation
(so every minimisation ends on its budget: a hop is a fixed amount of work), asynchronous (the default) and lockstep=True in
the same run.

    python scripts/bench_basinhopping.py [--mit 20] [--passes 5] [--pops 1,256,4096] [--ns 32,128] [--mfev 1000]

A pass is initialize() (the first minimisation) and run(mit), timed around both with a host clock: the run ends in a
device synchronise.  The first pass of a shape is a warm-up and is not counted.  "hop_share" is the share of device
time in bh_collect + bh_decide (the hop kernel's slots of the "profile" key over all slots), taken in one extra pass
with the profile on: event pairs slow the host, so that pass is not timed.  The rows report the passes' median with
their least and largest.  The reference's ms per hop on one host core comes from
scripts/gen_basinhopping_golden.py --time.  One JSON line per measurement; nothing is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))      # the package, when run as scripts/bench_basinhopping.py


def make(bb, kind, n, P, mit, mfev, lockstep):
    if kind == "nm":
        inner = bb.NelderMead(mfev, 1e-8, 0.5, seed=1, populations=P)
    else:
        inner = bb.Rosenbrock(mfev, 1e-8, 1., seed=1, populations=P)
    return bb.BasinHopping(inner, bb.BasinHopping_AdaptStrategy(0.1), False, mit, 1., seed=1, lockstep=lockstep)


def one_pass(bb, g, n, P, mit, profile=False):
    lo, up = -5. * np.ones(n), 5. * np.ones(n)
    guess = np.random.default_rng(n).uniform(-3., 3., P * n)
    t0 = time.perf_counter()
    g.initialize(bb.objectives.rosenbrock, lo, up, guess)
    if profile:
        g.set_state("profile", [1.])
    g.run(mit)
    return time.perf_counter() - t0


def measure(kind, n, P, lockstep, mit, mfev, passes):
    import bboptpy_amd as bb
    g = make(bb, kind, n, P, mit, mfev, lockstep)
    one_pass(bb, g, n, P, mit)
    dts = [one_pass(bb, g, n, P, mit) for _ in range(passes)]
    probe = range(0, P, max(1, P // 64))
    fev = float(np.mean([g.get_state("fev", p)[0] for p in probe]))
    one_pass(bb, g, n, P, mit, profile=True)
    prof = g.get_state("profile").reshape(-1, 2)[:, 0]      # ms: inner walk, hop, collect, decide, begin, evaluate
    dt = float(np.median(dts))
    return {"minimizer": kind, "n": n, "P": P, "lockstep": int(lockstep), "mit": mit, "mfev": mfev, "passes": passes,
            "ms_per_hop": 1e3 * dt / (mit + 1), "ms_per_hop_min_max": [1e3 * min(dts) / (mit + 1), 1e3 * max(dts) / (mit + 1)],
            "evals_per_chain": fev, "evals_per_s": fev * P / dt,
            "hop_share": float(prof[1:].sum() / prof.sum()) if prof.sum() > 0 else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mit", type=int, default=20)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--pops", default="1,256,4096")
    ap.add_argument("--ns", default="32,128")
    ap.add_argument("--mfev", type=int, default=1000)
    a = ap.parse_args()
    for n in (int(v) for v in a.ns.split(",")):
        for P in (int(v) for v in a.pops.split(",")):
            for kind in ("nm", "rosen"):
                for lockstep in (False, True):
                    print(json.dumps(measure(kind, n, P, lockstep, a.mit, a.mfev, a.passes)), flush=True)


if __name__ == "__main__":
    main()
