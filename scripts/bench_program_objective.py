#!/usr/bin/env python
"""What an objective program costs next to the built-in objective and the host batch callback
(DESIGN.md section 3.1 holds the numbers this prints).

  (a) ActiveCMAES n = 128, lambda = 4096, Rosenbrock: time per generation with the built-in, a
      program in staged form, a program in direct form, and a vectorised NumPy batch callback
  (b) SHADE n = 128, np = 4096, Rastrigin (the program calls cos)
  (c) the evaluation kernel alone (SepCMAES, lambda = 4096), n in {16, 64, 128, 256, 512}, both
      forms: bytes of X read per second

Cases of one part are timed in alternation, `--rounds` rounds after a warm-up of every case; the
figure kept is the median.  The callback case moves populations * lambda * n * 8 bytes each way per
generation: it runs at `--callback-populations` populations and is SCALED to `--populations`
(the line says so).  `--tree DIR` imports the package of another built checkout (with
`--callback-only`: the callback case of the commit before this feature).  One JSON line per figure.

    python scripts/bench_program_objective.py --parts a,b,c
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ROSEN_SRC = r"""
extern "C" __device__ double bbo_user_objective(const double *x, int n, const double *data)
{
    double s = 0.;
    for (int j = 0; j + 1 < n; j++) {
        const double t = x[j + 1] - x[j] * x[j], u = 1. - x[j];
        s += 100. * (t * t) + u * u;
    }
    return s;
}
"""

RASTRIGIN_SRC = r"""
extern "C" __device__ double bbo_user_objective(const double *x, int n, const double *data)
{
    double s = 0.;
    for (int j = 0; j < n; j++) s += x[j] * x[j] - 10. * cos(6.283185307179586 * x[j]);
    return 10. * n + s;
}
"""


def rosen_batch(X):
    return np.sum(100. * (X[:, 1:] - X[:, :-1] ** 2) ** 2 + (1. - X[:, :-1]) ** 2, axis=1)


def rastrigin_batch(X):
    return 10. * X.shape[1] + np.sum(X * X - 10. * np.cos(2. * np.pi * X), axis=1)


def emit(**rec):
    print(json.dumps(rec), flush=True)


def timed_run(g, gens):
    t0 = time.perf_counter()
    done = g.run(gens)
    dt = time.perf_counter() - t0
    assert done == gens, "the run stopped early (%d of %d generations)" % (done, gens)
    return dt / gens


def alternate(cases, gens, rounds, warmup):
    """cases: name -> (optimizer, generations per timed run); every case warmed, then round-robin"""
    for g, _ in cases.values():
        g.run(warmup)
    samples = {k: [] for k in cases}
    for _ in range(rounds):
        for k, (g, gn) in cases.items():
            samples[k].append(timed_run(g, gn))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in samples.items()}


def part_generation(bb, part, make, builtin, src, batch, box, args):
    n = args.n
    lo, up = box[0] * np.ones(n), box[1] * np.ones(n)
    rng = np.random.default_rng(1)
    cases = {}
    if not args.callback_only:
        prog = bb.DeviceObjective(src)
        for name, f, stage in (("builtin", builtin, None), ("program_staged", prog, 1), ("program_direct", prog, 0)):
            g = make(args.populations)
            g.initialize(f, lo, up, rng.uniform(box[0] / 2, box[1] / 2, n * args.populations))
            if stage is not None:
                g.set_state("prog_stage", [stage])
            cases[name] = (g, args.gens)
    g = make(args.callback_populations)
    g.initialize(bb.vectorized(batch), lo, up, rng.uniform(box[0] / 2, box[1] / 2, n * args.callback_populations))
    cases["batch_callback"] = (g, max(2, args.gens // 4))
    res = alternate(cases, args.gens, args.rounds, args.warmup)
    scale = args.populations / args.callback_populations
    for name, (med, lo_, hi_) in res.items():
        rec = dict(part=part, case=name, n=n, rows=args.rows, populations=args.populations,
                   ms_per_generation=1e3 * med, ms_min=1e3 * lo_, ms_max=1e3 * hi_, tree=args.tree or "this checkout")
        if name == "batch_callback":
            rec.update(ms_per_generation=1e3 * med * scale, ms_min=1e3 * lo_ * scale, ms_max=1e3 * hi_ * scale,
                       scaled=True, measured_populations=args.callback_populations,
                       note="measured at %d populations, multiplied by %g" % (args.callback_populations, scale))
        emit(**rec)
    if "builtin" in res:
        for name in ("program_staged", "program_direct"):
            emit(part=part, ratio=name + " / builtin", value=res[name][0] / res["builtin"][0])
            emit(part=part, ratio="batch_callback (scaled) / " + name, value=res["batch_callback"][0] * scale / res[name][0])


def part_kernel(bb, args):
    """the evaluation launch alone, by the engine's own event pair around it (get "prog_profile")"""
    prog = bb.DeviceObjective(ROSEN_SRC)
    rows, pops = args.rows, args.kernel_populations
    for n in (16, 64, 128, 256, 512):
        lo, up = -5. * np.ones(n), 5. * np.ones(n)
        handles = {}
        for stage in (1, 0):
            g = bb.SepCMAES(2 ** 30, 1e-300, rows, seed=7, populations=pops)
            g.initialize(prog, lo, up, np.zeros(n * pops))
            g.set_state("prog_stage", [stage])
            try:
                g.run(2)
            except Exception as e:      # (64 staged rows of this n do not fit LDS)
                emit(part="c", n=n, form="staged" if stage else "direct", unavailable=str(e).splitlines()[0])
                continue
            handles[stage] = g
        samples = {s: [] for s in handles}
        for _ in range(args.rounds):
            for s, g in handles.items():
                g.set_state("profile", [1.])
                g.run(args.kernel_gens)
                ms, calls = g.get_state("prog_profile")
                samples[s].append(ms / calls)
        for s, v in samples.items():
            med = statistics.median(v)
            nbytes = pops * rows * n * 8
            emit(part="c", n=n, form="staged" if s else "direct", rows=rows, populations=pops,
                 us_per_launch=1e3 * med, us_min=1e3 * min(v), us_max=1e3 * max(v),
                 x_bytes=nbytes, x_gb_per_s=nbytes / (med * 1e-3) / 1e9)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--rows", type=int, default=4096, help="lambda / np")
    ap.add_argument("--populations", type=int, default=256)
    ap.add_argument("--callback-populations", type=int, default=16)
    ap.add_argument("--kernel-populations", type=int, default=64)
    ap.add_argument("--gens", type=int, default=8)
    ap.add_argument("--kernel-gens", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--callback-only", action="store_true")
    ap.add_argument("--tree", default=None, help="root of another built checkout to import the package from")
    args = ap.parse_args()

    sys.path.insert(0, os.path.abspath(args.tree) if args.tree else ROOT)
    import bboptpy_amd as bb

    parts = args.parts.split(",")
    if "a" in parts:
        part_generation(bb, "a", lambda P: bb.ActiveCMAES(2 ** 30, 1e-300, args.rows, seed=11, populations=P,
                                                          poll_every=args.gens),
                        bb.objectives.rosenbrock, ROSEN_SRC, rosen_batch, (-5., 5.), args)
    if "b" in parts:
        part_generation(bb, "b", lambda P: bb.SHADE(2 ** 30, args.rows, 1e-300, seed=11, populations=P,
                                                    poll_every=args.gens),
                        bb.objectives.rastrigin, RASTRIGIN_SRC, rastrigin_batch, (-5.12, 5.12), args)
    if "c" in parts and not args.callback_only:
        part_kernel(bb, args)


if __name__ == "__main__":
    main()
