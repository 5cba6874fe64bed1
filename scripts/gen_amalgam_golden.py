#!/usr/bin/env python3
"""Records states of the REAL Amalgam of the reference into tests/golden/amalgam_runs.json (needs the
reference's sources and g++).

    python scripts/gen_amalgam_golden.py [--ref /root/reference] [--out tests/golden/amalgam_runs.json]
    python scripts/gen_amalgam_golden.py --time     (ms per generation of the reference at n = 128 on one
                                                     host core, for scripts/bench_amalgam.py's lines)

A small harness (the C++ text below, this project's own) is compiled in a temporary directory
against the reference's amalgam.cpp and blas.cpp with the flags of oracle/Makefile (-O2
-ffp-contract=off).  Every member of the class is protected and its distribution _Z is public, so a
probe subclass can read the whole state and replay the draws a generation is about to make on copies
of the engine and of the distribution.  The fixture holds numbers and names only; an array of floats
is ONE string, base64 of its little-endian IEEE doubles, scalars are float.hex strings.

"steps": the seed, from which tests/amalgam_model.py (reference_draws) regenerates the class's initial
points and the normals of generation 1 -- checked here against the class, bit for bit -- then per
later generation the np * n normals in sampling order (`z`), and per generation `perm`: the sampling row every position holds after the
shuffle of rows 1.., found by matching the rows the class holds after iterate() against mu + chol z
and that plus the shift.  The shifted rows are perm[1 : nams + 1].  The listed generations keep the
whole state: arx (up to n = 5; beyond, mu + chol z and fit_val pin the rows) and fit_val brought back to
sampling order, fit_idx (their stable ranking), mu,
mushift, cov, chol, cmult, nis, t, fev.
"pivot": the factor the class leaves of the crafted covariances of amalgam_model.crafted, whose
factorisation meets a non-positive pivot (etasigma is set to 0 in the probe, so updateDistribution keeps the crafted matrix).
"runs": outcomes (fev, converged, f of the returned point) of complete runs of iAMaLGaM on Rosenbrock
n = 10 in [-5, 5], stol = 1e-8: 16 seeds and one run that ends on the budget.
"noparam": three runs of the parameter-free mode: the rows the class printed, and per copy the
outcome of the same inner run made through the public interface (the harness checks that the two
agree in every printed row).

The seed of a "steps" run is advanced until no two fitness values of a recorded generation are
closer than 1e-9 relative.
"""
import argparse
import base64
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (name, n, objective, iamalgam, first seed, generations, recorded generations)
STEPS = [
    ("n2_iamalgam", 2, "rosenbrock", 1, 31, 5, [1, 2, 5]),
    ("n2_amalgam", 2, "rosenbrock", 0, 32, 5, [1, 2, 5]),
    ("n5_iamalgam", 5, "rosenbrock", 1, 33, 5, [1, 2, 5]),
    ("n5_amalgam", 5, "ellipsoid", 0, 34, 5, [1, 2, 5]),
    ("n17_amalgam", 17, "rosenbrock", 0, 35, 1, [1]),
    ("n33_iamalgam", 33, "rosenbrock", 1, 36, 1, [1]),
]
OBJ_IDS = {"sphere": 0, "rosenbrock": 1, "rastrigin": 2, "ellipsoid": 3, "ackley": 4,
           "griewank": 5, "cigar": 6, "discus": 7, "diffpow": 8, "schwefel12": 9}
RUN_SEEDS = list(range(501, 517))
RUN_N, RUN_STOL, RUN_MFEV = 10, 1e-8, 400000
BUDGET_RUN = (10, 1e-8, 2000, 531)      # n, stol, mfev, seed
# (n, iamalgam, tol, stol, mfev, seed): the last one's budget binds inside the two copies of stage 2
NOPARAM = [(4, 1, 1e-6, 1e-8, 200000, 541), (3, 0, 1e-8, 1e-8, 6000, 542), (5, 1, 0., 1e-8, 9000, 543)]
MIN_GAP = 1e-9
ARX_MAX_N = 5          # arx is kept up to this n; beyond, mu + chol z and fit_val pin the rows
STATE_KEYS = ("arx", "fit_val", "mu", "mushift", "cov", "chol", "cmult")

HARNESS = r"""
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "objectives.h"
#include "random.hpp"
#include "multivariate/amalgam/amalgam.h"

using Random = effolkronium::random_static;

static void vec(const char *k, const std::vector<double> &v)
{
    printf("\"%s\":[", k);
    for (size_t i = 0; i < v.size(); i++) printf("%s\"%a\"", i ? "," : "", v[i]);
    printf("],");
}

struct Probe: public Amalgam {
    using Amalgam::Amalgam;
    // the normals of the next iterate(), on copies of the engine and of the distribution
    void peek()
    {
        auto eng = Random::get_engine();
        auto dist = _Z;
        std::vector<double> z;
        for (int i = 0; i < _np * _n; i++) z.push_back(dist(eng));
        vec("z", z);
    }
    void points()
    {
        std::vector<double> arx, fv;
        for (auto &p : _sols) {
            arx.insert(arx.end(), p._x.begin(), p._x.end());
            fv.push_back(p._f);
        }
        vec("arx", arx); vec("fit_val", fv);
    }
    void dump()
    {
        std::vector<double> cov, chol;
        for (auto &r : _cov) cov.insert(cov.end(), r.begin(), r.end());
        for (auto &r : _chol) chol.insert(chol.end(), r.begin(), r.end());
        points();
        vec("mu", _mu); vec("mushift", _mushift); vec("cov", cov); vec("chol", chol); vec("cmult", { _cmult });
        printf("\"np\":%d,\"ss\":%d,\"nams\":%d,\"nis\":%d,\"t\":%d,\"fev\":%d,\"etasigma\":\"%a\",\"etashift\":\"%a\"",
                _np, _ss, _nams, _nis, _t, _fev, _etasigma, _etashift);
    }
    void craft(const std::vector<double> &m)
    {
        _etasigma = 0.;
        for (int i = 0; i < _n; i++)
            for (int j = 0; j < _n; j++) _cov[i][j] = m[i * _n + j];
    }
    int nbase() const { return _nbase; }
};

struct Ctx { int obj, n; std::vector<double> aux; long calls; };

int main(int argc, char **argv)
{
    // steps   <obj> <n> <iamalgam> <seed> <gens>
    // pivot   <n> <seed>            (the matrix, n * n hexadecimal doubles, on stdin)
    // run     <n> <stol> <mfev> <seed>
    // noparam <n> <iamalgam> <tol> <stol> <mfev> <seed>
    // time    <iamalgam> <n> <gens>
    const std::string mode = argv[1];
    const int n = mode == "steps" ? atoi(argv[3]) : mode == "time" ? atoi(argv[3]) : atoi(argv[2]);
    Ctx c { mode == "steps" ? atoi(argv[2]) : BBO_OBJ_ROSENBROCK, n, std::vector<double>(n, 0.), 0 };
    bbo_objective_aux(c.obj, n, c.aux.data());
    std::vector<double> lo(n, -5.), up(n, 5.), guess(n, 0.);
    multivariate f = [&c](const double *x) { c.calls++; return bbo_objective_eval(c.obj, c.n, x, c.aux.data()); };
    multivariate_problem prob { f, n, lo.data(), up.data() };
    if (mode == "time") {
        const int gens = atoi(argv[4]);
        Random::seed(1u);
        Probe p(1000000000, 0., 0., 0, atoi(argv[2]) != 0, false, false);
        p.init(prob, guess.data());
        p.iterate();
        const auto t0 = std::chrono::steady_clock::now();
        for (int g = 0; g < gens; g++) p.iterate();
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        printf("{\"n\":%d,\"iamalgam\":%d,\"generations\":%d,\"reference_ms_per_generation\":%.4f}\n", n, atoi(argv[2]),
                gens, ms / gens);
    } else if (mode == "steps") {
        const int gens = atoi(argv[6]);
        Random::seed((unsigned) atoi(argv[5]));
        Probe p(1000000000, 0., 0., 0, atoi(argv[4]) != 0, false, false);
        p.init(prob, guess.data());
        printf("{\"init\":{");
        p.dump();
        printf("},\"states\":[");
        for (int g = 1; g <= gens; g++) {
            printf("%s{\"gen\":%d,", g > 1 ? "," : "", g);
            p.peek();
            p.iterate();
            p.dump();
            printf("}");
        }
        printf("]}\n");
    } else if (mode == "pivot") {
        Random::seed((unsigned) atoi(argv[3]));
        Probe p(1000000000, 0., 0., 0, false, false, false);
        p.init(prob, guess.data());
        std::vector<double> m(n * n);
        for (auto &v : m) {
            char buf[64];
            if (scanf("%63s", buf) != 1) return 2;
            v = strtod(buf, nullptr);
        }
        p.craft(m);
        p.iterate();
        printf("{");
        p.dump();
        printf("}\n");
    } else if (mode == "run") {
        Random::seed((unsigned) atoi(argv[5]));
        Probe p(atoi(argv[4]), 0., atof(argv[3]), 0, true, false, false);
        const auto sol = p.optimize(prob, guess.data());
        const long calls = c.calls;     // (the class's own, before the harness evaluates the result)
        printf("{\"seed\":%d,\"fev\":%d,\"converged\":%d,\"f\":\"%a\",\"calls\":%ld}\n", atoi(argv[5]), sol._fev,
                sol._converged ? 1 : 0, f(sol._sol.data()), calls);
    } else {
        const bool iam = atoi(argv[3]) != 0;
        const double tol = atof(argv[4]), stol = atof(argv[5]);
        const int mfev = atoi(argv[6]);
        const unsigned seed = (unsigned) atoi(argv[7]);
        // the class itself, printing its table
        Random::seed(seed);
        Probe p(mfev, tol, stol, 0, iam, true, true);
        const auto sol = p.optimize(prob, guess.data());
        printf("{\"fev\":%d,\"converged\":%d,\"f\":\"%a\",\"nbase\":%d,\"copies\":[", sol._fev, sol._converged ? 1 : 0,
                f(sol._sol.data()), p.nbase());
        // the same copies through the public interface, as runParallel makes them (:257-288)
        Random::seed(seed);
        int budget = mfev, fev = 0, first = 1;
        double fbestrun = 1. / 0., fbestrunold;
        for (int s = 0;; s++) {
            const int half = s >> 1;
            const int np = (s & 1) ? (1 << (1 + half)) * p.nbase() : (1 + half) * p.nbase();
            const int runs = (s & 1) ? 1 : 1 << half;
            fbestrunold = fbestrun;
            fbestrun = 1. / 0.;
            for (int r = 0; r < runs; r++) {
                Amalgam algr { budget, tol, stol, np, iam, false, false };
                const auto so = algr.optimize(prob, nullptr);
                const double fitr = f(so._sol.data());
                printf("%s{\"s\":%d,\"r\":%d,\"np\":%d,\"cap\":%d,\"fev\":%d,\"f\":\"%a\"}", first ? "" : ",", s, r, np,
                        budget, so._fev, fitr);
                first = 0;
                fev += so._fev + 1;
                budget -= so._fev + 1;
                if (fitr < fbestrun) fbestrun = fitr;
            }
            if (fev >= mfev) break;
            if (fbestrun != fbestrunold && std::fabs(fbestrun - fbestrunold) <= tol) break;
        }
        printf("],\"emulated_fev\":%d}\n", fev);
    }
    return 0;
}
"""


def _floats(hexes):
    return [float.fromhex(v) for v in hexes]


def _pack(values):
    """a list of floats as base64 of their little-endian IEEE doubles"""
    values = [float(v) for v in np.asarray(values, dtype=np.float64).ravel()]
    return base64.b64encode(struct.pack("<%dd" % len(values), *values)).decode()


def _min_gap(values):
    """smallest relative gap between neighbours of the sorted values"""
    v = sorted(values)
    gap = float("inf")
    for a, b in zip(v, v[1:]):
        gap = min(gap, (b - a) / max(abs(a), abs(b), 1e-300))
    return gap


def _build(ref, tmp):
    src = os.path.join(ref, "src")
    with open(os.path.join(tmp, "harness.cpp"), "w") as fh:
        fh.write(HARNESS)
    exe = os.path.join(tmp, "harness")
    subprocess.check_call(
        ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-w", "-I" + src,
         "-I" + os.path.join(ROOT, "oracle"), "-o", exe, os.path.join(tmp, "harness.cpp"),
         os.path.join(src, "blas.cpp"), os.path.join(src, "multivariate/amalgam/amalgam.cpp"), "-lm"])
    return exe


def time_reference(ref="/root/reference"):
    tmp = tempfile.mkdtemp(prefix="amalgam_golden_")
    try:
        exe = _build(ref, tmp)
        for iam, gens in ((1, 20), (0, 2)):
            print(subprocess.check_output([exe, "time", str(iam), "128", str(gens)]).decode().strip(), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _perm(st, prev_cmult, n, np_):
    """position after the shuffle -> sampling row: the row the class holds at position k is
    mu + chol z_m, or that plus 2 cmult mushift, for exactly one m"""
    z = np.array(_floats(st["z"])).reshape(np_, n)
    mu, chol = np.array(_floats(st["mu"])), np.array(_floats(st["chol"])).reshape(n, n)
    shift = 2. * prev_cmult * np.array(_floats(st["mushift"]))
    pre = mu[None, :] + z @ chol.T
    post = np.array(_floats(st["arx"])).reshape(np_, n)
    scale = max(1., float(np.abs(post).max()))
    perm = []
    for k in range(np_):
        d = np.minimum(np.abs(post[k][None, :] - pre).max(axis=1), np.abs(post[k][None, :] - shift - pre).max(axis=1))
        m = int(np.argmin(d))
        assert d[m] < 1e-9 * scale, (k, d[m])
        perm.append(m)
    assert sorted(perm) == list(range(np_)) and perm[0] == 0
    return perm


def generate(ref="/root/reference"):
    import amalgam_model as model
    tmp = tempfile.mkdtemp(prefix="amalgam_golden_")
    try:
        exe = _build(ref, tmp)
        steps = []
        for name, n, obj, iam, seed0, gens, recorded in STEPS:
            for seed in range(seed0, seed0 + 50 * 100, 100):
                out = subprocess.check_output([exe, "steps", str(OBJ_IDS[obj]), str(n), str(iam), str(seed), str(gens)])
                rec = json.loads(out)
                if all(_min_gap(_floats(st["fit_val"])) > MIN_GAP
                       for st in [rec["init"]] + rec["states"] if st is rec["init"] or st["gen"] in recorded):
                    break
                print("%s: seed %d has fitness values closer than %g, trying the next" % (name, seed, MIN_GAP))
            else:
                sys.exit("%s: no tie-free seed" % name)
            init = rec.pop("init")
            np_ = init["np"]
            x0, z1 = model.reference_draws(seed, n, np_, model.objective(obj, n))
            assert _floats(init["arx"]) == [float(v) for v in x0.ravel()], name
            consts = {k: init[k] for k in ("np", "ss", "nams", "etasigma", "etashift")}
            prev_cmult = 1.
            for st in rec["states"]:
                perm = _perm(st, prev_cmult, n, np_)
                prev_cmult = _floats(st["cmult"])[0]
                z = _floats(st.pop("z"))
                if st["gen"] == 1:
                    assert z == [float(v) for v in z1.ravel()], name
                if st["gen"] in recorded:
                    inv = np.argsort(perm)          # sampling row -> position
                    arx = np.array(_floats(st["arx"])).reshape(np_, n)[inv]
                    fv = np.array(_floats(st["fit_val"]))[inv]
                    st["fit_idx"] = [int(i) for i in model.rank_order(fv)]
                    st["arx"], st["fit_val"] = _pack(arx), _pack(fv)
                    if n > ARX_MAX_N:
                        del st["arx"]
                    for k in STATE_KEYS[2:]:
                        st[k] = _pack(_floats(st[k]))
                else:
                    for k in STATE_KEYS + ("nis", "t", "fev"):
                        del st[k]
                for k in ("np", "ss", "nams", "etasigma", "etashift"):
                    del st[k]
                if st["gen"] > 1:
                    st["z"] = _pack(z)
                st["perm"] = perm
            rec.update(consts)
            rec.update({"name": name, "n": n, "objective": obj, "iamalgam": iam, "seed": seed, "recorded": recorded,
                        "mu0": _pack(_floats(init["mu"])), "cov0": _pack(_floats(init["cov"]))})
            steps.append(rec)

        pivots = []
        for n, rank in ((8, 5), (20, 17)):
            a = model.crafted(n, rank, 1e-3)
            out = subprocess.check_output([exe, "pivot", str(n), "7"],
                                          input=" ".join(float(v).hex() for v in a.ravel()).encode())
            st = json.loads(out)
            _, fail = model.dchdc(a)
            assert fail == rank, (n, fail)
            assert _floats(st["cov"]) == [float(v) for v in a.ravel()]      # the probe kept the crafted matrix
            pivots.append({"n": n, "rank": rank, "drop": 1e-3, "fail_at": fail, "chol": _pack(_floats(st["chol"]))})

        def run(n, stol, mfev, seed):
            r = json.loads(subprocess.check_output([exe, "run", str(n), repr(stol), str(mfev), str(seed)]))
            r["f"] = float.fromhex(r["f"]).hex()
            return r

        budget = run(*BUDGET_RUN)
        budget.update({"n": BUDGET_RUN[0], "stol": BUDGET_RUN[1], "mfev": BUDGET_RUN[2]})
        runs = {"objective": "rosenbrock", "n": RUN_N, "stol": RUN_STOL, "mfev": RUN_MFEV, "iamalgam": 1,
                "converging": [run(RUN_N, RUN_STOL, RUN_MFEV, s) for s in RUN_SEEDS], "budget": budget}

        noparam = []
        for n, iam, tol, stol, mfev, seed in NOPARAM:
            out = subprocess.check_output(
                [exe, "noparam", str(n), str(iam), repr(tol), repr(stol), str(mfev), str(seed)]).decode()
            lines = out.splitlines()
            table = [ln for ln in lines if ln.startswith(" |")]
            r = json.loads([ln for ln in lines if ln.startswith("{")][0])
            assert r["emulated_fev"] == r["fev"], (r["emulated_fev"], r["fev"])
            rows = model.parameter_free(r["nbase"], mfev, tol, _replay(r["copies"]))
            import _tabular
            widths = [5, 5, 10, 25, 25, 10]
            want = [_tabular.fmt_row(["iter", "runs", "pop", "f*", "best f*", "fev"], widths), _tabular.rule(widths)]
            want += [_tabular.fmt_row(list(row), widths) for row in rows]
            assert want == table, "\n".join(want + ["--"] + table)
            r.update({"n": n, "iamalgam": iam, "tol": tol, "stol": stol, "mfev": mfev, "seed": seed, "table": table})
            r["f"] = float.fromhex(r["f"]).hex()
            for cp in r["copies"]:
                cp["f"] = float.fromhex(cp["f"]).hex()
            noparam.append(r)
        return {"steps": steps, "pivot": pivots, "runs": runs, "noparam": noparam}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _replay(copies):
    it = iter(copies)

    def inner(s, r, np_, cap):
        cp = next(it)
        assert (cp["s"], cp["r"], cp["np"], cp["cap"]) == (s, r, np_, cap), (cp, s, r, np_, cap)
        return cp["fev"], float.fromhex(cp["f"])
    return inner


def dumps(data):
    return json.dumps(data, sort_keys=True, separators=(",", ":")) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "amalgam_runs.json"))
    ap.add_argument("--time", action="store_true", help="time the reference instead of writing the fixture")
    a = ap.parse_args()
    if not os.path.isdir(os.path.join(a.ref, "src")):
        sys.exit("the reference sources are not at %s" % a.ref)
    if a.time:
        time_reference(a.ref)
        return
    text = dumps(generate(a.ref))
    with open(a.out, "w") as fh:
        fh.write(text)
    print("wrote %s (%d bytes)" % (a.out, len(text)))


if __name__ == "__main__":
    main()
