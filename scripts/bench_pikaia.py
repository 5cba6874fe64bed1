#!/usr/bin/env python3
"""PIKAIA throughput on one GPU: ms per generation of the whole handle and evaluations per second at n = 128,
nd = 6 on Rosenbrock over [-5, 5]^n, for np = 256 x {1, 256, 4096} populations and np = 4096 x {1, 256}.

    python scripts/bench_pikaia.py [--passes 5] [--quick]

  generation   bbo_run: a generation is np evaluations (the counter says np + 1, as the reference's does) in
               three launches: pikaia_breed (np / 2 matings, the values of both children inside), pikaia_newpop
               (ranking, adjmut, the running sums of select; one workgroup per population), pikaia_copy
  breeding     the breeding kernel alone (its slot of "profile") at nd = 4, 8 and 9: one, two and three Philox
               calls per coordinate and child, the same bytes.  "breed_gbs" is the bytes of the two parent rows
               read and the four rows written (phenotypes and mapped points of both children) over its time;
               "bound" says "philox" when the time follows the calls (nd = 9 over nd = 4 beyond 1.5), "hbm"
               when the bytes move at more than half of the 8 TB/s peak, and "neither" otherwise: the kernel
               then waits on its own dependent chain (the draws of the mating, two bisections over the running
               sums, the parent rows, the stores, the rows read back for the values)

Each figure is the median of `passes` spans with the least and the largest next to it.  The reference's ms per
generation on one host core comes from scripts/gen_pikaia_golden.py --time.  One JSON line per measurement;
nothing is asserted."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))      # the package, when run as scripts/bench_pikaia.py

N = 128
NAMES = ("init", "breed", "newpop", "copy")
HBM_PEAK_GBS = 8000.


def start(P, np_, nd):
    import bboptpy_amd as bb
    g = bb.PIKAIA(np_, 2 ** 18, nd, seed=1, populations=P)
    g.initialize(bb.objectives.rosenbrock, -5. * np.ones(N), 5. * np.ones(N), np.zeros(P * N))
    return g


def profile(g, gens):
    g.set_state("profile", [1.])
    g.run(gens)
    prof = g.get_state("profile").reshape(-1, 2)
    g.set_state("profile", [0.])
    return {k: float(prof[i, 0]) / gens for i, k in enumerate(NAMES) if prof[i, 1] > 0}


def measure(P, np_, nd, gens, warmup, passes):
    g = start(P, np_, nd)
    g.run(warmup)
    dts = []
    for _ in range(passes):
        t0 = time.perf_counter()
        g.run(gens)
        dts.append(time.perf_counter() - t0)
    dt = float(np.median(dts))
    kern = profile(g, gens)
    total = sum(kern.values())
    return {"what": "generation", "P": P, "n": N, "np": np_, "nd": nd, "objective": "rosenbrock", "generations": gens,
            "warmup": warmup, "passes": passes, "evaluations_per_generation": np_,
            "ms_per_generation": 1e3 * dt / gens,
            "ms_per_generation_min_max": [1e3 * min(dts) / gens, 1e3 * max(dts) / gens],
            "evals_per_s": P * np_ * gens / dt,
            "kernel_ms_per_generation": kern, "breed_share": kern.get("breed", 0.) / total if total else 0.}


def breeding(P, np_, gens):
    """the breeding kernel against the Philox calls it issues"""
    out = {"what": "breeding", "P": P, "n": N, "np": np_, "generations": gens}
    nbytes = P * (np_ // 2) * 6 * N * 8
    ms = {}
    for nd in (4, 8, 9):
        g = start(P, np_, nd)
        g.run(gens)
        ms[nd] = profile(g, gens)["breed"]
    out["breed_ms_by_nd"] = {str(k): v for k, v in ms.items()}
    out["philox_calls_per_coordinate_and_child"] = {"4": 1, "8": 2, "9": 3}
    out["breed_gbs"] = {str(k): nbytes / (v * 1e-3) / 1e9 for k, v in ms.items()}
    out["philox_calls_per_s_nd9"] = P * np_ * N * 3 / (ms[9] * 1e-3)
    out["hbm_peak_share"] = max(out["breed_gbs"].values()) / HBM_PEAK_GBS
    out["bound"] = "philox" if ms[9] > 1.5 * ms[4] else "hbm" if out["hbm_peak_share"] > 0.5 else "neither"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="np = 256 only")
    a = ap.parse_args()
    shapes = [(256, 1), (256, 256), (256, 4096)] + ([] if a.quick else [(4096, 1), (4096, 256)])
    for np_, P in shapes:
        gens = 64 if P * np_ <= 256 * 256 else 8
        print(json.dumps(measure(P, np_, 6, gens, gens, a.passes)), flush=True)
    print(json.dumps(breeding(4096, 256, 8)), flush=True)
    if not a.quick:
        print(json.dumps(breeding(1, 4096, 64)), flush=True)


if __name__ == "__main__":
    main()
