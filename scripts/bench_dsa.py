#!/usr/bin/env python3
"""DSA throughput on one GPU: ms per generation, evaluations per second and the time per kernel
at n = 128, np = 4096, Rastrigin, for P = 256 populations of one handle and for P = 1.

    python scripts/bench_dsa.py [--steps 50] [--warmup 10] [--ref /root/reference]

Two passes per shape after the warm-up generations: one unprofiled (wall clock around run(), which
ends with a stream synchronisation) and one with the engine's `profile` switch (an event pair
around every launch on the engine's own stream: time per kernel).  dsa_evolve's bytes are counted
as 24 n per member -- its own row and its direction row read, its next row written -- and set
against the 8 TB/s HBM peak of the MI355X.  Where the reference's sources are present (--ref), its
DSSearch is also timed on one host core at the same shape, through the harness of
scripts/gen_dsa_golden.py.  One JSON line per measurement; nothing is asserted."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

HBM_PEAK = 8.0e12
SLOTS = ("dsa_rank", "dsa_plan", "dsa_evolve", "dsa_finish")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))      # the package, when run as scripts/bench_dsa.py


def measure(P, n, np_, steps, warmup):
    import bboptpy_amd as bb
    lo, up = -5.12 * np.ones(n), 5.12 * np.ones(n)
    g = bb.DSA(2 ** 31 - 1, 0., 0., np_, seed=1, populations=P, poll_every=steps)
    g.initialize(bb.objectives.rastrigin, lo, up, np.zeros((P, n)))
    g.run(warmup)
    t0 = time.perf_counter()
    g.run(steps)
    dt = time.perf_counter() - t0
    g.set_state("profile", [1.])
    g.run(steps)
    prof = g.get_state("profile").reshape(-1, 2)
    per = {name: 1e3 * prof[i, 0] / max(prof[i, 1], 1.) for i, name in enumerate(SLOTS)}   # us per launch
    evolve_s = per["dsa_evolve"] * 1e-6
    return {"P": P, "n": n, "np": np_, "objective": "rastrigin", "steps": steps,
            "evals_per_s": P * np_ * steps / dt, "ms_per_generation": 1e3 * dt / steps,
            "kernel_us": per,
            "evolve_bytes_per_s": P * np_ * n * 24 / evolve_s,
            "evolve_fraction_of_hbm_peak": P * np_ * n * 24 / evolve_s / HBM_PEAK}


def reference(ref, n, np_, gens):
    """the reference's DSSearch::optimize on one core: gens generations after the initial pool"""
    sys.path.insert(0, HERE)
    import gen_dsa_golden as gold
    tmp = tempfile.mkdtemp(prefix="dsa_bench_")
    try:
        exe = gold.build(ref, tmp)
        args = [exe, "bands", str(gold.OBJ_IDS["rastrigin"]), str(n), str(np_), str(np_ * (gens + 1)),
                "0.0", "0.0", "5.12", "1", "1"]
        t0 = time.perf_counter()
        subprocess.check_output(args[:5] + [str(np_)] + args[6:])       # the initial pool alone
        t_init = time.perf_counter() - t0
        t0 = time.perf_counter()
        subprocess.check_output(args)
        dt = time.perf_counter() - t0 - t_init
        return {"reference": "DSSearch, one host core", "n": n, "np": np_, "generations": gens,
                "ms_per_generation": 1e3 * dt / gens, "evals_per_s": np_ * gens / dt}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--reference-only", action="store_true")
    a = ap.parse_args()
    if not a.reference_only:
        for P in (256, 1):
            print(json.dumps(measure(P, 128, 4096, a.steps, a.warmup)))
    if os.path.isdir(os.path.join(a.ref, "src")):
        print(json.dumps(reference(a.ref, 128, 4096, 20)))


if __name__ == "__main__":
    main()
