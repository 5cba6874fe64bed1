#!/usr/bin/env python3
"""Records runs of the REAL NelderMead of the reference into tests/golden/neldermead_runs.json (needs the
reference's sources and g++; run on the development machine, never where the GPU tests run).

    python scripts/gen_neldermead_golden.py [--ref /root/reference] [--out tests/golden/neldermead_runs.json]
    python scripts/gen_neldermead_golden.py --time     # the reference's us per simplex step on one core

A small harness (the C++ text below, this project's own) is compiled in a temporary directory against the
reference's nelder_mead.cpp with the flags of oracle/Makefile (-O2 -ffp-contract=off).  It drives a subclass
probe; initSimplex() and nelmin() are private members, so the harness reads the class's header with `private`
spelt `protected` (the layout of the object does not depend on it).

  steps   init(), the first simplex as nelmin()'s first pass builds and evaluates it, then 20 calls of the
          reference's iterate(): after each the whole of _p and _y, _ihi, _ilo, _ylo, _icount, _jcount, _conv,
          and every point handed to the objective with its value, in order
  run     optimize() whole: every point and value in order, xmin, the count and the verdict
  coef    _ccoef, _ecoef, _rcoef, _scoef (from std::cos) per (pinit, n)

Every recorded run is replayed here through tests/neldermead_model.py and must match bit for bit: the points,
the values, the state after every step, the result.  What the fixture keeps: per step the model's branch (the
state that follows pins it), ihi, ilo, icount, jcount, conv, CRC-32 sums of p and y and of the points and values
of the step, and whether the step is "ok" -- one the device's built-in objective can be held to: none of its
comparisons (ystar against ylo and every y, y2star against ystar or y[ihi], the maximum against the runner-up,
sumsq against rq) is within 1e-6 relative of a tie.  A shape's start point moves (by 0.0625 per coordinate, at
most 40 times) until 12 of its 20 steps are ok.  Per whole run: the result, the CRC-32 of all points and values,
the events of nelmin() (stop test fired, factorial test passed or failed with the probes counted, restart,
budget exit).  Every path must be met at least twice over the fixture (the wide simplexes, rad0 = 4, on
Rosenbrock are there for the shrink and the refused outside contraction).
"signature": the argument names and defaults of the constructor in nelder_mead.h; "enums": the names of the
two enums in order.  Floats are float.hex strings.  The fixture holds numbers and names only.
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (name, n, objective, minit, pinit, base of the start point)
STEP_SHAPES = [
    ("n2_axis_original", 2, "rosenbrock", "coordinate_axis", "original", -1.25),
    ("n3_spendley_gao", 3, "sphere", "spendley", "gao2010", 1.5),
    ("n17_pfeffer_crude", 17, "rosenbrock", "pfeffer", "mehta2019_crude", 0.75),
    ("n33_spendley_refined", 33, "rosenbrock", "spendley", "mehta2019_refined", -0.5),
    ("n65_axis_refined", 65, "sphere", "coordinate_axis", "mehta2019_refined", 2.25),
    ("n128_spendley_refined", 128, "rosenbrock", "spendley", "mehta2019_refined", 0.5),
]
# (name, n, objective, minit, pinit, start base, mfev, tol, rad0, checkev, eps)
RUN_SHAPES = [
    ("run_n1_spendley", 1, "sphere", "spendley", "mehta2019_refined", 1.5, 400, 1e-8, 1., 10, 1e-3),
    ("run_n1_axis", 1, "sphere", "coordinate_axis", "gao2010", -0.75, 400, 1e-8, 0.5, 3, 1e-3),
    ("run_n2_rosen", 2, "rosenbrock", "spendley", "mehta2019_refined", -1.25, 4000, 1e-8, 1., 10, 1e-3),
    ("run_n3_sphere", 3, "sphere", "coordinate_axis", "original", 1.5, 4000, 1e-8, 0.5, 10, 1e-3),
    ("run_n2_loose", 2, "rosenbrock", "pfeffer", "gao2010", -1.25, 3000, 0.5, 1., 5, 1e-3),
    ("run_n3_loose", 3, "sphere", "spendley", "mehta2019_crude", 1.5, 3000, 1., 1., 4, 1e-2),
    ("run_n2_wide", 2, "rosenbrock", "coordinate_axis", "mehta2019_refined", -3., 3000, 1e-8, 4., 10, 1e-3),
    ("run_n3_wide", 3, "rosenbrock", "coordinate_axis", "original", -3., 3000, 1e-8, 4., 10, 1e-3),
    ("run_n2_refuse", 2, "rosenbrock", "pfeffer", "mehta2019_crude", -3., 3000, 1e-8, 4., 10, 1e-3),
    ("run_n3_refuse", 3, "rosenbrock", "spendley", "gao2010", -1.25, 3000, 1e-8, 1., 10, 1e-3),
    ("run_n17_budget", 17, "rosenbrock", "spendley", "mehta2019_refined", 0.75, 2500, 1e-8, 1., 10, 1e-3),
    ("run_n33_budget", 33, "sphere", "pfeffer", "gao2010", -0.5, 1500, 1e-8, 1., 10, 1e-3),
    ("run_n65_budget", 65, "rosenbrock", "coordinate_axis", "mehta2019_crude", 2.25, 900, 1e-8, 0.5, 10, 1e-3),
    ("run_n128_budget", 128, "rosenbrock", "spendley", "mehta2019_refined", 0.5, 700, 1e-8, 1., 10, 1e-3),
]
STEPS, GOOD_OK, STARTS_TRIED, START_SHIFT = 20, 12, 40, 0.0625
STEP_PARAMS = dict(mfev=1 << 20, tol=1e-8, rad0=1., checkev=10, eps=1e-3)
OBJ_IDS = {"sphere": 0, "rosenbrock": 1}

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
#include <string>
#include <vector>
#include "objectives.h"
#include "random.hpp"
#include "multivariate/multivariate.h"
#define private protected
#include "multivariate/simplex/nelder_mead.h"
#undef private

static void vec(const char *k, const std::vector<double> &v)
{
    printf("\"%s\":[", k);
    for (size_t i = 0; i < v.size(); i++) printf("%s\"%a\"", i ? "," : "", v[i]);
    printf("],");
}

struct Probe: public NelderMead {
    using NelderMead::NelderMead;
    // nelmin()'s first pass (:251-260)
    void first()
    {
        initSimplex();
        for (int j = 0; j <= _n; j++) _y[j] = _f._f(&(_p[j])[0]);
        _icount += (_n + 1);
        _ilo = std::min_element(_y.begin(), _y.end()) - _y.begin() + 1;
        _ylo = _y[_ilo - 1];
    }
    void dump()
    {
        std::vector<double> flat;
        for (auto &r : _p) flat.insert(flat.end(), r.begin(), r.end());
        vec("p", flat);
        vec("y", _y);
        printf("\"ihi\":%d,\"ilo\":%d,\"ylo\":\"%a\",\"icount\":%d,\"jcount\":%d,\"conv\":%d", _ihi - 1, _ilo - 1, _ylo,
                _icount, _jcount, _conv ? 1 : 0);
    }
    void coef() { printf("[\"%a\",\"%a\",\"%a\",\"%a\"]\n", _ccoef, _ecoef, _rcoef, _scoef); }
};

int main(int argc, char **argv)
{
    // steps <obj> <n> <minit> <pinit> <mfev> <tol> <rad0> <checkev> <eps> <steps> <start...>
    // run   <obj> <n> <minit> <pinit> <mfev> <tol> <rad0> <checkev> <eps> 0       <start...>
    // time  <obj> <n> <minit> <pinit> <mfev> <tol> <rad0> <checkev> <eps> <steps> <start...>
    // coef  <obj> <n> <minit> <pinit>
    const int obj = atoi(argv[2]), n = atoi(argv[3]);
    std::vector<double> aux(n), log;
    bool keep = true;
    bbo_objective_aux(obj, n, aux.data());
    multivariate f = [&](const double *x) {
        const double v = bbo_objective_eval(obj, n, x, aux.data());
        if (keep) {
            log.insert(log.end(), x, x + n);
            log.push_back(v);
        }
        return v;
    };
    std::vector<double> lo(n, -5.), up(n, 5.), guess(n, 0.);
    multivariate_problem prob { f, n, lo.data(), up.data() };
    const auto minit = (NelderMead::simplex_initializer) atoi(argv[4]);
    const auto pinit = (NelderMead::parameter_initializer) atoi(argv[5]);
    if (!strcmp(argv[1], "coef")) {
        Probe p(100, 1e-8, 1., minit, pinit);
        p.init(prob, guess.data());
        p.coef();
        return 0;
    }
    const int steps = atoi(argv[11]);
    for (int j = 0; j < n; j++) guess[j] = strtod(argv[12 + j], nullptr);
    Probe p(atoi(argv[6]), strtod(argv[7], nullptr), strtod(argv[8], nullptr), minit, pinit, atoi(argv[9]),
            strtod(argv[10], nullptr));
    if (!strcmp(argv[1], "steps")) {
        p.init(prob, guess.data());
        p.first();
        printf("{\"init\":{");
        vec("evals", log);
        p.dump();
        printf("},\"states\":[");
        for (int g = 0; g < steps; g++) {
            log.clear();
            p.iterate();
            printf("%s{", g ? "," : "");
            vec("evals", log);
            p.dump();
            printf("}");
        }
        printf("]}\n");
    } else if (!strcmp(argv[1], "run")) {
        const multivariate_solution sol = p.optimize(prob, guess.data());
        printf("{");
        vec("evals", log);
        vec("x", sol._sol);
        printf("\"icount\":%d,\"converged\":%d}\n", sol._fev, sol._converged ? 1 : 0);
    } else {
        keep = false;
        p.init(prob, guess.data());
        p.first();
        for (int g = 0; g < 10; g++) p.iterate();
        const auto t0 = std::chrono::steady_clock::now();
        for (int g = 0; g < steps; g++) p.iterate();
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        printf("{\"us_per_step\":%.6f}\n", us / steps);
    }
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
         os.path.join(src, "multivariate/simplex/nelder_mead.cpp"), "-lm"])
    return exe


def start_point(n, base, attempt):
    """a start off every symmetry (no two coordinates alike, no period: a repeated pattern makes vertices
    tie exactly on Rosenbrock): the base, a scatter, and the shift of the attempt"""
    return [base + 0.5 * (((37 * j * j + 11 * j) % 127) / 127.) + START_SHIFT * attempt for j in range(n)]


def call(exe, mode, obj, n, minit, pinit, par, steps, guess):
    import neldermead_model as nm
    out = subprocess.check_output(
        [exe, mode, str(OBJ_IDS[obj]), str(n), str(nm.MINIT[minit]), str(nm.PINIT[pinit]), str(par["mfev"]),
         repr(par["tol"]), repr(par["rad0"]), str(par["checkev"]), repr(par["eps"]), str(steps)]
        + [float(v).hex() for v in guess])
    return json.loads(out)


def model_of(obj, n, minit, pinit, par):
    import chol_model
    import neldermead_model as nm
    return nm.Model(chol_model.objective(obj, n), n, par["mfev"], par["tol"], par["rad0"], nm.MINIT[minit],
                    nm.PINIT[pinit], par["checkev"], par["eps"])


def flat_evals(m):
    return [v for x, fx in m.evals for v in x + [fx]]


def replay_steps(rec, shape, guess):
    import neldermead_model as nm
    name, n, obj, minit, pinit, _ = shape
    m = model_of(obj, n, minit, pinit, STEP_PARAMS)

    def same(st, tag):
        assert flat_evals(m) == _hx(st["evals"]), tag + "evals"
        assert [v for r in m.p for v in r] == _hx(st["p"]), tag + "p"
        assert m.y == _hx(st["y"]), tag + "y"
        assert (m.ilo, m.ylo, m.icount, m.jcount, int(m.conv)) == (
            st["ilo"], float.fromhex(st["ylo"]), st["icount"], st["jcount"], st["conv"]), tag + "scalars"

    m.init(guess)
    m.first_simplex()
    same(rec["init"], name + " init ")
    out = {"name": name, "n": n, "objective": obj, "minit": minit, "pinit": pinit, "guess": [v.hex() for v in guess],
           "params": dict(STEP_PARAMS), "init": {"state_crc": m.state_crc(), "ilo": m.ilo, "icount": m.icount},
           "states": []}
    for g, st in enumerate(rec["states"]):
        m.evals = []
        m.iterate()
        tag = "%s step %d " % (name, g)
        same(st, tag)
        assert m.ihi == st["ihi"], tag + "ihi"
        out["states"].append({"branch": m.branch, "ihi": m.ihi, "ilo": m.ilo, "icount": m.icount, "jcount": m.jcount,
                              "conv": int(m.conv), "state_crc": m.state_crc(), "evals_crc": nm.crc(flat_evals(m)),
                              "nevals": len(m.evals), "ok": bool(m.ok())})
    out["paths"] = dict(m.paths)
    return out


def record_steps(exe, shape):
    name, n, obj, minit, pinit, base = shape
    for attempt in range(STARTS_TRIED):
        guess = start_point(n, base, attempt)
        out = replay_steps(call(exe, "steps", obj, n, minit, pinit, STEP_PARAMS, STEPS, guess), shape, guess)
        if sum(st["ok"] for st in out["states"]) >= GOOD_OK:
            return out
    sys.exit("%s: no start of %d with %d comparable steps" % (name, STARTS_TRIED, GOOD_OK))


def record_run(exe, shape):
    import neldermead_model as nm
    name, n, obj, minit, pinit, base, mfev, tol, rad0, checkev, eps = shape
    par = dict(mfev=mfev, tol=tol, rad0=rad0, checkev=checkev, eps=eps)
    guess = start_point(n, base, 0)
    rec = call(exe, "run", obj, n, minit, pinit, par, 0, guess)
    m = model_of(obj, n, minit, pinit, par)
    x, icount, conv = m.optimize(guess)
    assert flat_evals(m) == _hx(rec["evals"]), name + ": the points and values of the run"
    assert x == _hx(rec["x"]) and icount == rec["icount"] and int(conv) == rec["converged"], name + ": the result"
    return {"name": name, "n": n, "objective": obj, "minit": minit, "pinit": pinit, "guess": [v.hex() for v in guess],
            "params": par, "x": [v.hex() for v in x], "icount": icount, "converged": int(conv),
            "evals_crc": nm.crc(flat_evals(m)), "nevals": len(m.evals), "steps": m.it, "restarts": m.restarts,
            "events": [list(e) for e in m.events], "paths": dict(m.paths)}


def signature(ref):
    """the argument names and defaults of the constructor (nelder_mead.h:58-60) and the enums' names"""
    with open(os.path.join(ref, "src", "multivariate", "simplex", "nelder_mead.h"), errors="replace") as fh:
        text = " ".join(fh.read().split())
    body = re.search(r"NelderMead\(([^)]*)\);", text).group(1)
    sig = []
    for arg in body.split(","):
        mt = re.match(r"\s*(\w+)\s+(\w+)\s*(?:=\s*([\w.+-]+))?\s*$", arg)
        kind, name, default = mt.groups()
        if default is None:
            sig.append({"name": name, "required": True})
        elif kind in ("int", "double"):
            sig.append({"name": name, "required": False, "default": float(default) if kind == "double" else int(default)})
        else:
            sig.append({"name": name, "required": False, "default": default})
    enums = {}
    for mt in re.finditer(r"enum (\w+) \{([^}]*)\}", text):
        enums[mt.group(1)] = [v.strip() for v in mt.group(2).split(",")]
    return sig, enums


def generate(ref="/root/reference"):
    import neldermead_model as nm
    tmp = tempfile.mkdtemp(prefix="neldermead_golden_")
    try:
        exe = build(ref, tmp)
        have = {k: 0 for k in nm.PATHS}
        steps, runs = [], []
        for shape in STEP_SHAPES:
            steps.append(record_steps(exe, shape))
        for shape in RUN_SHAPES:
            runs.append(record_run(exe, shape))
        for rec in steps + runs:
            for k in nm.PATHS:
                have[k] += rec["paths"][k]
        for k in nm.PATHS:
            if have[k] < 2:
                sys.exit("path %s met %d times only (all: %s)" % (k, have[k], have))
        coef = {}
        for pinit, pid in nm.PINIT.items():
            for n in sorted({s[1] for s in STEP_SHAPES} | {1}):
                got = json.loads(subprocess.check_output([exe, "coef", "0", str(n), "1", str(pid)]))
                assert _hx(got) == list(nm.coefficients(pid, n)), "coef %s n = %d" % (pinit, n)
                coef["%s:%d" % (pinit, n)] = got
        sig, enums = signature(ref)
        return {"steps": steps, "runs": runs, "paths": have, "coef": coef, "signature": sig, "enums": enums}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def time_reference(ref="/root/reference"):
    """us per simplex step of the reference on one core: the shapes of scripts/bench_neldermead.py"""
    tmp = tempfile.mkdtemp(prefix="neldermead_time_")
    try:
        exe = build(ref, tmp)
        par = dict(mfev=1 << 30, tol=0., rad0=1., checkev=10, eps=1e-3)
        for n, steps in ((32, 20000), (128, 5000)):
            guess = start_point(n, -2., 0)
            runs = [call(exe, "time", "rosenbrock", n, "spendley", "mehta2019_refined", par, steps, guess)
                    for _ in range(5)]
            us = sorted(r["us_per_step"] for r in runs)
            print("n = %d: %.3f us per simplex step (median of 5 runs of %d steps; least %.3f, largest %.3f)"
                  % (n, us[2], steps, us[0], us[-1]))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def dumps(data):
    return json.dumps(data, sort_keys=True, separators=(",", ":")) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "neldermead_runs.json"))
    ap.add_argument("--time", action="store_true")
    a = ap.parse_args()
    if not os.path.isdir(os.path.join(a.ref, "src")):
        sys.exit("the reference sources are not at %s" % a.ref)
    if a.time:
        time_reference(a.ref)
        return
    data = generate(a.ref)
    text = dumps(data)
    with open(a.out, "w") as fh:
        fh.write(text)
    for rec in data["steps"]:
        print("%s: ok %d of %d, paths %s" % (rec["name"], sum(s["ok"] for s in rec["states"]), len(rec["states"]),
                                            {k: v for k, v in rec["paths"].items() if v}))
    for rec in data["runs"]:
        print("%s: %d evaluations, %d steps, converged %d, events %s" % (rec["name"], rec["icount"], rec["steps"],
                                                                        rec["converged"], rec["events"][-6:]))
    print("paths over the fixture: %s" % data["paths"])
    print("wrote %s (%d bytes)" % (a.out, len(text)))


if __name__ == "__main__":
    main()
