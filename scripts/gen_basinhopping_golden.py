#!/usr/bin/env python3
"""Records runs of the REAL BasinHopping of the reference, over its NelderMead and its Rosenbrock, into
tests/golden/basinhopping_runs.json (needs the reference's sources and g++; run on the development machine, never
where the GPU tests run).

    python scripts/gen_basinhopping_golden.py [--ref /root/reference] [--out tests/golden/basinhopping_runs.json]
    python scripts/gen_basinhopping_golden.py --time    # the reference's ms per hop on one core

A small harness (the C++ text below, this project's own) is compiled in a temporary directory against the
reference's basinhopping.cpp, nelder_mead.cpp, rosenbrock.cpp and blas.cpp with the flags of oracle/Makefile
(-O2 -ffp-contract=off).  It seeds the global generator (Random::seed(k)) and hands BasinHopping a minimiser that
passes every optimize() on to the real one and notes the start, the result, the count and the verdict.  The draws of
a hop are read from a copy of the engine taken before iterate(): n values of uniform_real_distribution(-1, 1), one
of (0, 1), after which the copy must equal the engine (the minimisers draw nothing).  The table the reference prints
is parsed for it, f, conv, step, accept, f* and fev.

Every recorded run is replayed through tests/basinhopping_model.py on the recorded draws and must match bit for bit
before it is written: the rows, the starts, the results, the counts, the best point.  A hop is close when
|w - u| < 1e-9 (the device's exp may round the other way): the seed of a run moves until no hop of it is close, and
the fixture stores the count (0).  Over the fixture the generator asserts inner runs that end on the budget and
inner runs that converge, both values of accept, both directions of the adaptive adjustment and coordinates of a
step that hit either clamp at least twice (the n = 17 shapes start near the box's edges for that).
"global": Rastrigin n = 2 on [-5.12, 5.12], NelderMead, `chains` model chains of 8 hops from seeded uniform starts
with the draws of bbo_bh_draws -- the chains whose first minimisation / whose best lies in the global basin
(f < 0.5), for the seed (of six) where the hops gain most over the first minimisations alone.  Floats are float.hex
strings.  Points are CRC-32 sums, the start and the result of every hop too (in full they are nine tenths of a
fixture of 326 KB), and the draws are not kept: tests/basinhopping_model.py regenerates the reference's generator
from the seed, which is held here to the draws read from the engine; the tests replay the model for the points.
Numbers and names only.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)     # ("global": the draws come from the built library, bbo_bh_draws)

MIT = 8
SIZE_CAP = 466942       # bytes, the cap of scripts/gen_acd_golden.py
OBJ_IDS = {"sphere": 0, "rosenbrock": 1, "rastrigin": 2}
SEEDS_TRIED = 40
NM = dict(kind="nm", tol=1e-8, rad0=0.5)
ROSEN = dict(kind="rosen", tol=1e-6, step0=0.5, decf=0.1)
PLAIN = dict(adaptive=0, stepsize=0.1, accept_rate=0.5, interval=5, factor=0.9)
ADAPT = dict(adaptive=1, stepsize=0.25, accept_rate=0.5, interval=2, factor=0.9)
# (name, n, objective, box, start base, minimiser, its mfev, strategy, temp, optimize() calls on one strategy object)
SHAPES = []
for _n, _obj, _box, _base, _budgets in ((2, "rosenbrock", 5., -1.25, (400, 2000)), (17, "rastrigin", 5.12, 4.4, (1500, 4000))):
    for _mk, _mn, _mfev in (("nm", NM, _budgets[0]), ("rosen", ROSEN, _budgets[1])):
        for _sk, _st in (("plain", PLAIN), ("adapt", ADAPT)):
            SHAPES.append(("n%d_%s_%s_%s" % (_n, _obj, _mk, _sk), _n, _obj, _box, _base, _mn, _mfev, _st, 1., 1))
# (the sizes of the 128-thread workgroups: the sphere at n = 65, Rosenbrock at n = 128)
for _n, _obj, _base, _budgets in ((65, "sphere", 2.25, (800, 4000)), (128, "rosenbrock", 0.5, (400, 4000))):
    for _mk, _mn, _mfev in (("nm", NM, _budgets[0]), ("rosen", ROSEN, _budgets[1])):
        for _sk, _st in (("plain", PLAIN), ("adapt", ADAPT)):
            SHAPES.append(("n%d_%s_%s_%s" % (_n, _obj, _mk, _sk), _n, _obj, 5., _base, _mn, _mfev, _st, 1., 1))
SHAPES += [("n2_temp0_rosen", 2, "rosenbrock", 5., -1.25, ROSEN, 2000, ADAPT, 0., 1),
           ("n17_temp0_nm", 17, "rastrigin", 5.12, -4.9, NM, 1500, ADAPT, 0., 1),
           ("n2_reused_nm", 2, "rosenbrock", 5., -1.25, NM, 400, ADAPT, 1., 2)]
# (48 chains: the model walks them in seconds, and a callable-driven device run of them stays a few seconds)
GLOBAL = dict(n=2, box=5.12, chains=48, mit=MIT, mfev=400, tol=1e-8, rad0=0.5, stepsize=0.12, temp=1.)
GLOBAL_SEEDS = 6

HARNESS = r"""
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <iostream>
#include <numeric>
#include <random>
#include <sstream>
#include <string>
#include <vector>
#include "objectives.h"
#include "random.hpp"
#include "multivariate/multivariate.h"
#include "multivariate/simplex/nelder_mead.h"
#include "multivariate/rosenbrock/rosenbrock.h"
#include "multivariate/basin/basinhopping.h"

using Random = effolkronium::random_static;

static void vec(const char *k, const std::vector<double> &v)
{
    printf("\"%s\":[", k);
    for (size_t i = 0; i < v.size(); i++) printf("%s\"%a\"", i ? "," : "", v[i]);
    printf("],");
}

// passes optimize() on and notes what went in and what came out
struct Noting: public MultivariateOptimizer {
    MultivariateOptimizer *in;
    int n = 0;
    std::vector<double> start, sol;
    int fev = 0, conv = 0;
    explicit Noting(MultivariateOptimizer *m) : in(m) {}
    void init(const multivariate_problem &f, const double *guess) override { in->init(f, guess); }
    void iterate() override { in->iterate(); }
    multivariate_solution solution() override { return in->solution(); }
    multivariate_solution optimize(const multivariate_problem &f, const double *guess) override
    {
        n = f._n;
        start.assign(guess, guess + n);
        const multivariate_solution s = in->optimize(f, guess);
        sol = s._sol;
        fev = s._fev;
        conv = s._converged ? 1 : 0;
        return s;
    }
};

struct Probe: public BasinHopping {
    using BasinHopping::BasinHopping;
    int it() const { return _it; }
    int fev() const { return _fev; }
    double energy() const { return _energy; }
    double best() const { return _bestenergy; }
    const std::vector<double> &x() const { return _x; }
    const std::vector<double> &bestx() const { return _bestx; }
};

int main(int argc, char **argv)
{
    // run|time <obj> <n> <box> <seed> <mit> <temp> <kind> <mfev> <tol> <rad0|step0> <decf> <adaptive> <stepsize>
    //          <accept_rate> <interval> <factor> <calls> <start...>
    const int obj = atoi(argv[2]), n = atoi(argv[3]);
    const double box = strtod(argv[4], nullptr);
    std::vector<double> aux(n);
    bbo_objective_aux(obj, n, aux.data());
    multivariate f = [&](const double *x) { return bbo_objective_eval(obj, n, x, aux.data()); };
    std::vector<double> lo(n, -box), up(n, box), guess(n, 0.);
    multivariate_problem prob { f, n, lo.data(), up.data() };
    const int mit = atoi(argv[6]), mfev = atoi(argv[9]), calls = atoi(argv[18]);
    const double temp = strtod(argv[7], nullptr), tol = strtod(argv[10], nullptr), a0 = strtod(argv[11], nullptr);
    for (int j = 0; j < n; j++) guess[j] = strtod(argv[19 + j], nullptr);
    NelderMead nmin(mfev, tol, a0);
    Rosenbrock rmin(mfev, tol, a0, strtod(argv[12], nullptr));
    Noting noting(!strcmp(argv[8], "nm") ? (MultivariateOptimizer*) &nmin : (MultivariateOptimizer*) &rmin);
    StepsizeStrategy plain(strtod(argv[14], nullptr));
    AdaptiveStepsizeStrategy adapt(strtod(argv[14], nullptr), strtod(argv[15], nullptr), atoi(argv[16]),
            strtod(argv[17], nullptr));
    StepsizeStrategy *strat = atoi(argv[13]) ? (StepsizeStrategy*) &adapt : &plain;
    Random::seed((unsigned) atoi(argv[5]));
    if (!strcmp(argv[1], "time")) {
        Probe p(&noting, strat, false, mit, temp);
        p.init(prob, guess.data());
        const auto t0 = std::chrono::steady_clock::now();
        while (p.it() < mit) p.iterate();
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        printf("{\"ms_per_hop\":%.6f,\"fev\":%d}\n", ms / mit, p.fev());
        return 0;
    }
    printf("{\"calls\":[");
    for (int call = 0; call < calls; call++) {
        // the table goes to std::cout: caught per call and handed on as text
        std::ostringstream table;
        std::streambuf *old = std::cout.rdbuf(table.rdbuf());
        Probe p(&noting, strat, true, mit, temp);
        p.init(prob, guess.data());
        printf("%s{\"hops\":[{", call ? "," : "");
        vec("start", noting.start); vec("sol", noting.sol);
        printf("\"inner_fev\":%d,\"conv\":%d,\"step\":\"%a\"}", noting.fev, noting.conv, strat->_stepsize);
        while (p.it() < mit) {
            auto copy = Random::get_engine();
            std::vector<double> draws;
            for (int j = 0; j < n; j++) draws.push_back(std::uniform_real_distribution<double>(-1., 1.)(copy));
            draws.push_back(std::uniform_real_distribution<double>(0., 1.)(copy));
            const double before = p.energy();
            p.iterate();
            if (!(copy == Random::get_engine())) {
                std::cout.rdbuf(old);
                fprintf(stderr, "the engine moved by another count than n + 1 draws\n");
                return 2;
            }
            printf(",{");
            vec("draws", draws); vec("start", noting.start); vec("sol", noting.sol);
            printf("\"inner_fev\":%d,\"conv\":%d,\"step\":\"%a\",\"energy_before\":\"%a\",\"energy\":\"%a\",\"best\":\"%a\","
                    "\"fev\":%d}", noting.fev, noting.conv, strat->_stepsize, before, p.energy(), p.best(), p.fev());
        }
        std::cout.rdbuf(old);
        printf("],");
        vec("xbest", p.bestx()); vec("x", p.x());
        std::string text = table.str(), esc;
        for (char ch : text) esc += ch == '\n' ? std::string("\\n") : std::string(1, ch);
        printf("\"fev\":%d,\"table\":\"%s\"}", p.fev(), esc.c_str());
    }
    printf("]}\n");
    return 0;
}
"""


def _hx(v):
    return [float.fromhex(s) for s in v]


def build(ref, tmp):
    src = os.path.join(ref, "src")
    with open(os.path.join(tmp, "harness.cpp"), "w") as fh:
        fh.write(HARNESS)
    exe = os.path.join(tmp, "harness")
    subprocess.check_call(
        ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-w", "-include", "cmath", "-I" + src,
         "-I" + os.path.join(ROOT, "oracle"), "-o", exe, os.path.join(tmp, "harness.cpp"),
         os.path.join(src, "multivariate/basin/basinhopping.cpp"),
         os.path.join(src, "multivariate/simplex/nelder_mead.cpp"),
         os.path.join(src, "multivariate/rosenbrock/rosenbrock.cpp"), os.path.join(src, "blas.cpp"), "-lm"])
    return exe


def start_point(n, base):
    return [base + 0.0625 * (i % 7) for i in range(n)]


def call(exe, mode, shape, seed, mit=MIT):
    name, n, obj, box, base, mn, mfev, st, temp, calls = shape
    a0 = mn["rad0"] if mn["kind"] == "nm" else mn["step0"]
    out = subprocess.check_output(
        [exe, mode, str(OBJ_IDS[obj]), str(n), repr(box), str(seed), str(mit), repr(temp), mn["kind"], str(mfev),
         repr(mn["tol"]), repr(a0), repr(mn.get("decf", 0.1)), str(st["adaptive"]), repr(st["stepsize"]),
         repr(st["accept_rate"]), str(st["interval"]), repr(st["factor"]), str(calls)]
        + [float(v).hex() for v in start_point(n, base)])
    return json.loads(out)


def minimizer_of(shape, f):
    import basinhopping_model as bm
    name, n, obj, box, base, mn, mfev, st, temp, calls = shape
    if mn["kind"] == "nm":
        return bm.nm_minimizer(f, n, mfev, mn["tol"], mn["rad0"])
    return bm.rosen_minimizer(f, n, mfev, mn["tol"], mn["step0"], mn["decf"])


def strategy_of(st):
    import basinhopping_model as bm
    if st["adaptive"]:
        return bm.Strategy(st["stepsize"], st["accept_rate"], st["interval"], st["factor"])
    return bm.Strategy(st["stepsize"])


def parse_table(text):
    """the rows of the reference's table: it, f, conv, step, accept, f*, fev"""
    rows = []
    for line in text.split("\n")[2:]:
        cells = [c.strip() for c in line.split("|")[1:-1]]
        if len(cells) == 7:
            rows.append([int(cells[0]), float(cells[1]), int(cells[2]), float(cells[3]), int(cells[4]),
                         float(cells[5]), int(cells[6])])
    return rows


def replay(rec, shape, seed):
    """the recorded calls through the model; the fixture's record of the run, or None when a hop is close"""
    import basinhopping_model as bm
    import rosenbrock_model as rm
    name, n, obj, box, base, mn, mfev, st, temp, calls = shape
    f = rm.objective(obj, n)
    strat = strategy_of(st)
    guess = start_point(n, base)
    out = {"name": name, "n": n, "objective": obj, "box": box, "base": base, "seed": seed,
           "minimizer": dict(mn, mfev=mfev), "strategy": dict(st), "temp": temp, "mit": MIT, "calls": []}
    for k, c in enumerate(rec["calls"]):
        tag = "%s call %d " % (name, k)
        m = bm.Model(f, [-box] * n, [box] * n, minimizer_of(shape, f), strat, MIT, temp)
        nstep0, naccept0, step0 = strat.nstep, strat.naccept, strat.stepsize
        table = [_hx(h["draws"]) for h in c["hops"][1:]]
        # the draws are not kept: the tests regenerate them from the seed, the calls of a run in one stream
        assert table == bm.reference_draws(seed, n, MIT * (k + 1))[MIT * k:], tag + "the draws from the seed"
        xbest, fev, conv = m.optimize(guess, table)
        printed = parse_table(c["table"])
        assert len(printed) == len(m.rows) == MIT + 1, tag + "rows"
        for r, h, pr in zip(m.rows, c["hops"], printed):
            t = tag + "row %d " % r["it"]
            assert r["start"] == _hx(h["start"]), t + "start"
            assert r["sol"] == _hx(h["sol"]), t + "sol"
            assert (r["inner_fev"], r["conv"]) == (h["inner_fev"], h["conv"]), t + "the minimiser's count and verdict"
            assert r["step"] == float.fromhex(h["step"]), t + "step"
            assert [r["it"], r["f"], r["conv"], r["step"], r["accept"], r["fbest"], r["fev"]] == pr, t + "the table"
        assert xbest == _hx(c["xbest"]) and m.x == _hx(c["x"]) and fev == c["fev"], tag + "the result"
        if m.close():
            return None
        out["calls"].append({
            "nstep0": nstep0, "naccept0": naccept0, "stepsize0": step0.hex(),
            "rows": [{"it": r["it"], "f": r["f"].hex(), "conv": r["conv"], "step": r["step"].hex(), "accept": r["accept"],
                      "fbest": r["fbest"].hex(), "fev": r["fev"], "inner_fev": r["inner_fev"],
                      "start_crc": rm.crc(r["start"]), "sol_crc": rm.crc(r["sol"])} for r in m.rows],
            # the results that are the zero vector; the coordinates of the hops' starts on the upper / lower clamp
            "zeros": sum(not any(r["sol"]) for r in m.rows),
            "clamped": [sum(v == side * (box - 0.05 * (box + box)) for r in m.rows[1:] for v in r["start"])
                        for side in (1., -1.)],
            "xbest_crc": rm.crc(xbest), "x_crc": rm.crc(m.x), "fev": fev,
            "nstep": strat.nstep, "naccept": strat.naccept, "stepsize": strat.stepsize.hex(), "close": 0})
    return out


def record(exe, shape):
    for seed in range(1, SEEDS_TRIED + 1):
        out = replay(call(exe, "run", shape, seed), shape, seed)
        if out is not None:
            return out
    sys.exit("%s: every seed of %d has a close decision" % (shape[0], SEEDS_TRIED))


def coverage(runs):
    have = {"budget": 0, "converged": 0, "accepted": 0, "rejected": 0, "widened": 0, "narrowed": 0,
            "clamped_above": 0, "clamped_below": 0}
    for rec in runs:
        for c in rec["calls"]:
            rows = c["rows"]
            have["clamped_above"] += c["clamped"][0]
            have["clamped_below"] += c["clamped"][1]
            for k, r in enumerate(rows):
                have["converged" if r["conv"] else "budget"] += 1
                if k:
                    have["accepted" if r["accept"] else "rejected"] += 1
                    a, b = float.fromhex(rows[k - 1]["step"]), float.fromhex(r["step"])
                    have["widened"] += b > a
                    have["narrowed"] += b < a
    return have


def global_chains(seed, chains=None):
    """the model's chains of the "global" case: the draws of bbo_bh_draws, uniform starts from numpy's generator"""
    import numpy as np
    import basinhopping_model as bm
    import rosenbrock_model as rm
    from bboptpy_amd import BasinHopping
    g = GLOBAL
    n, box, P = g["n"], g["box"], chains or g["chains"]
    f = rm.objective("rastrigin", n)
    starts = np.random.default_rng(seed).uniform(-box, box, (P, n))
    first = best = 0
    for p in range(P):
        m = bm.Model(f, [-box] * n, [box] * n, bm.nm_minimizer(f, n, g["mfev"], g["tol"], g["rad0"]),
                     bm.Strategy(g["stepsize"]), g["mit"], g["temp"])
        m.optimize(list(starts[p]), [list(BasinHopping.draws(seed, p, hop, n)) for hop in range(g["mit"])])
        first += m.rows[0]["f"] < 0.5
        best += m.fbest < 0.5
    return int(first), int(best)


def fix_global():
    """The seed of GLOBAL_SEEDS whose chains gain most over their own first minimisations.  No setting tried puts a
    majority of the 48 chains into the global basin within 8 hops: over stepsize 0.06, 0.09, 0.12, 0.18, 0.25 x temp
    0.3, 1, 3 x seeds 1 to 3 the most were 12 (stepsize 0.12, temp 1, seed 2), against 0 or 1 first minimisations.
    About one start in fifty lands there and a hop reaches the neighbouring basins."""
    found = max((global_chains(seed)[::-1] + (seed,) for seed in range(1, GLOBAL_SEEDS + 1)),
                key=lambda t: (t[0] - t[1], -t[2]))
    best, first, seed = found
    if best <= first:
        sys.exit("no seed whose chains reach the global basin more often than their first minimisations")
    return dict(GLOBAL, seed=seed, first_in_global_basin=first, best_in_global_basin=best)


def generate(ref="/root/reference"):
    tmp = tempfile.mkdtemp(prefix="basinhopping_golden_")
    try:
        exe = build(ref, tmp)
        runs = [record(exe, shape) for shape in SHAPES]
        have = coverage(runs)
        for k, v in have.items():
            if v < 2:
                sys.exit("%s met %d times only (all: %s)" % (k, v, have))
        return {"runs": runs, "coverage": have, "close": 0, "global": fix_global()}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def time_reference(ref="/root/reference"):
    """ms per hop of the reference on one core: the shapes of scripts/bench_basinhopping.py"""
    tmp = tempfile.mkdtemp(prefix="basinhopping_time_")
    try:
        exe = build(ref, tmp)
        for n in (32, 128):
            for mn, mfev in ((dict(kind="nm", tol=1e-8, rad0=0.5), 1000), (dict(kind="rosen", tol=1e-8, step0=1., decf=0.1), 1000)):
                shape = ("time", n, "rosenbrock", 5., -2., mn, mfev, dict(ADAPT, stepsize=0.1, interval=5), 1., 1)
                ms = sorted(call(exe, "time", shape, 1, mit=20)["ms_per_hop"] for _ in range(5))
                print("n = %d, %s: %.3f ms per hop (median of 5 runs of 20 hops; least %.3f, largest %.3f)"
                      % (n, mn["kind"], ms[2], ms[0], ms[-1]))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def dumps(data):
    return json.dumps(data, sort_keys=True, separators=(",", ":")) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "basinhopping_runs.json"))
    ap.add_argument("--time", action="store_true")
    a = ap.parse_args()
    if not os.path.isdir(os.path.join(a.ref, "src")):
        sys.exit("the reference sources are not at %s" % a.ref)
    if a.time:
        time_reference(a.ref)
        return
    data = generate(a.ref)
    text = dumps(data)
    if len(text) > SIZE_CAP:
        sys.exit("the fixture would be %d bytes, over the cap of %d" % (len(text), SIZE_CAP))
    with open(a.out, "w") as fh:
        fh.write(text)
    for rec in data["runs"]:
        for c in rec["calls"]:
            print("%s (seed %d): fev %d, accepted %d of %d, converged inner runs %d of %d"
                  % (rec["name"], rec["seed"], c["fev"], sum(r["accept"] for r in c["rows"][1:]), MIT,
                     sum(r["conv"] for r in c["rows"]), MIT + 1))
    print("coverage: %s" % data["coverage"])
    print("global: %s" % data["global"])
    print("wrote %s (%d bytes)" % (a.out, len(text)))


if __name__ == "__main__":
    main()
