#!/usr/bin/env python3
"""Records runs of the REAL Rosenbrock of the reference into tests/golden/rosenbrock_runs.json (needs the
reference's sources and g++; run on the development machine, never where the GPU tests run).

    python scripts/gen_rosenbrock_golden.py [--ref /root/reference] [--out tests/golden/rosenbrock_runs.json]
    python scripts/gen_rosenbrock_golden.py --time     # the reference's us per line search on one core

A small harness (the C++ text below, this project's own) is compiled in a temporary directory against the
reference's rosenbrock.cpp and blas.cpp with the flags of oracle/Makefile (-O2 -ffp-contract=off).  It drives a
subclass probe; lineSearch() is a private member, so the harness reads the class's header with `private` spelt
`protected` (the layout of the object does not depend on it).

  steps   init(), `skip` calls of iterate(), then 24 more: after each the whole of _x, _v and _d, _stepi, _i, _fev,
          _ierr, _fs, and every point handed to the objective with its value, in order
  run     optimize() whole: every point and value in order, x, the count and the verdict

A window begins at search max(0, n + 1 - 12), so that it holds the first extra search and the first
orthogonalisation.  The Rastrigin shape meets both rare ends of the interpolation, imin 0 within its first 126
searches (its usual window holds one) and imin 3 from search 257 on, never in one window: a second window of
that shape begins where the model first meets imin 3 twice.  The first stage of the n = 17 shape moves less than
the step and shrinks it, so its usual window holds no orthogonalisation: a second window of that shape begins
where the model first meets one on an ok search.  Every recorded run is replayed here through tests/rosenbrock_model.py and must match
bit for bit: the points, the values, the state after every search, the result.  What the fixture keeps: per search
i before and after, fev, stepi, d[i], the path (direction 1 forward / 2 backward / 3 straight to the
interpolation, rounds of the doubling loop, imin, end 0 none / 1 kept / 2 restored / 3 budget), whether Palmer's
orthogonalisation ran, CRC-32 sums of x, v and d and of the points and values of the search, and whether the
search is "ok" -- one the device's built-in objective can be held to: none of its deciding comparisons (forward
against fx0, backward against fx0, each doubling against its predecessor, the two smallest of fs, the final value
against fs[imin]) is within 1e-6 relative of a tie.  A shape's start point moves (by 0.0625 per coordinate, at most
40 times) until 16 of its 24 searches are ok.  Per whole run: the result, the CRC-32 of all points and values, the
searches, the orthogonalisations, the paths.  Every path must be met at least twice over the fixture.
"signature": the argument names and defaults of the constructor in rosenbrock.h.  Floats are float.hex strings.
The fixture holds numbers and names only.
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

# (name, n, objective, base of the start point, step0)
STEP_SHAPES = [
    ("n2_rosen", 2, "rosenbrock", -1.25, 1.),
    ("n17_rosen", 17, "rosenbrock", 0.75, 1.),
    ("n17_rosen_orth", 17, "rosenbrock", 0.75, 1.),
    ("n33_rosen", 33, "rosenbrock", -0.5, 1.),
    ("n128_rosen", 128, "rosenbrock", 0.5, 1.),
    ("n65_sphere", 65, "sphere", 2.25, 1.),
    ("n128_rastrigin", 128, "rastrigin", 0.5, 1.5),
    ("n128_rastrigin_rare", 128, "rastrigin", 0.5, 1.5),
]
# (name, n, objective, start base, mfev, tol, step0, decf)
RUN_SHAPES = [
    ("run_n1_sphere", 1, "sphere", 1.5, 1 << 20, 1e-8, 1., 0.1),
    ("run_n3_sphere", 3, "sphere", 1.5, 1 << 20, 1e-8, 1., 0.1),
    ("run_n65_sphere", 65, "sphere", 2.25, 1 << 20, 1e-8, 1., 0.1),
    ("run_n128_sphere", 128, "sphere", 0.5, 1 << 20, 1e-8, 1., 0.1),
    ("run_n2_rosen", 2, "rosenbrock", -1.25, 1 << 20, 1e-8, 1., 0.1),
    ("run_n17_rosen", 17, "rosenbrock", 0.75, 1 << 20, 1e-8, 1., 0.1),
    ("run_n2_loose", 2, "rosenbrock", -1.25, 1 << 20, 1e-3, 0.5, 0.1),
    ("run_n128_budget", 128, "rosenbrock", 0.5, 3000, 1e-8, 1., 0.1),
    ("run_n1_constant", 1, "rosenbrock", 0.5, 400, 1e-8, 1., 0.1),
]
WINDOW, GOOD_OK, STARTS_TRIED, START_SHIFT = 24, 16, 40, 0.0625
RARE_SCAN = 400         # searches the model walks to find the window of a "_rare" or "_orth" shape
SIZE_CAP = 466942       # bytes, the cap of scripts/gen_acd_golden.py
STEP_PARAMS = dict(mfev=1 << 24, tol=1e-8, decf=0.1)
OBJ_IDS = {"sphere": 0, "rosenbrock": 1, "rastrigin": 2}

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
#include <string>
#include <vector>
#include "objectives.h"
#include "multivariate/multivariate.h"
#define private protected
#include "multivariate/rosenbrock/rosenbrock.h"
#undef private

static void vec(const char *k, const std::vector<double> &v)
{
    printf("\"%s\":[", k);
    for (size_t i = 0; i < v.size(); i++) printf("%s\"%a\"", i ? "," : "", v[i]);
    printf("],");
}

static std::vector<double> flat(const std::vector<std::vector<double>> &m)
{
    std::vector<double> f;
    for (auto &r : m) f.insert(f.end(), r.begin(), r.end());
    return f;
}

struct Probe: public Rosenbrock {
    using Rosenbrock::Rosenbrock;
    void dump()
    {
        vec("x", flat(_x));
        vec("v", flat(_v));
        vec("d", _d);
        vec("fs", _fs);
        printf("\"stepi\":\"%a\",\"i\":%d,\"fev\":%d,\"ierr\":%d", _stepi, _i, _fev, _ierr);
    }
    int ierr() const { return _ierr; }
};

int main(int argc, char **argv)
{
    // steps <obj> <n> <mfev> <tol> <step0> <decf> <skip> <count> <start...>
    // run   <obj> <n> <mfev> <tol> <step0> <decf> 0      0       <start...>
    // time  <obj> <n> <mfev> <tol> <step0> <decf> <skip> <count> <start...>
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
    const int skip = atoi(argv[8]), count = atoi(argv[9]);
    for (int j = 0; j < n; j++) guess[j] = strtod(argv[10 + j], nullptr);
    Probe p(atoi(argv[4]), strtod(argv[5], nullptr), strtod(argv[6], nullptr), strtod(argv[7], nullptr));
    if (!strcmp(argv[1], "steps")) {
        p.init(prob, guess.data());
        for (int g = 0; g < skip; g++) p.iterate();
        log.clear();
        printf("{\"before\":{");
        p.dump();
        printf("},\"states\":[");
        for (int g = 0; g < count && p.ierr() < 0; g++) {
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
        printf("\"fev\":%d,\"converged\":%d}\n", sol._fev, sol._converged ? 1 : 0);
    } else {
        keep = false;
        p.init(prob, guess.data());
        for (int g = 0; g < skip; g++) p.iterate();
        const auto t0 = std::chrono::steady_clock::now();
        int done = 0;
        for (; done < count && p.ierr() < 0; done++) p.iterate();
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        printf("{\"us_per_search\":%.6f,\"searches\":%d}\n", us / done, done);
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
         os.path.join(src, "multivariate/rosenbrock/rosenbrock.cpp"), os.path.join(src, "blas.cpp"), "-lm"])
    return exe


def start_point(n, base, attempt=0):
    return [base + 0.0625 * (i % 7) + START_SHIFT * attempt for i in range(n)]


def call(exe, mode, obj, n, par, skip, count, guess):
    out = subprocess.check_output(
        [exe, mode, str(OBJ_IDS[obj]), str(n), str(par["mfev"]), repr(par["tol"]), repr(par["step0"]),
         repr(par["decf"]), str(skip), str(count)] + [float(v).hex() for v in guess])
    return json.loads(out)


def model_of(obj, n, par):
    import rosenbrock_model as rm
    return rm.Model(rm.objective(obj, n), n, par["mfev"], par["tol"], par["step0"], par["decf"])


def flat_evals(m):
    return [v for x, fx in m.evals for v in x + [fx]]


def window_start(shape, par, guess):
    """the search a shape's window begins at"""
    name, n, obj, _, _ = shape
    if not name.endswith(("_rare", "_orth")):
        return max(0, n + 1 - 12)
    m = model_of(obj, n, par)
    m.init(guess)
    imins, oks, orths = [], [], []
    for _ in range(RARE_SCAN):
        m.iterate()
        imins.append(m.path[2])
        oks.append(m.ok())
        orths.append(m.orth and m.ok())
    for k in range(RARE_SCAN - WINDOW + 1):
        w = imins[k:k + WINDOW]
        found = w.count(3) >= 2 if name.endswith("_rare") else any(orths[k + WINDOW // 2:k + WINDOW])
        if found and sum(oks[k:k + WINDOW]) >= GOOD_OK:
            return k
    return None


def replay_steps(rec, shape, par, skip, guess):
    import rosenbrock_model as rm
    name, n, obj, _, _ = shape
    m = model_of(obj, n, par)

    def same(st, tag):
        assert m.flat(m.x) == _hx(st["x"]), tag + "x"
        assert m.flat(m.v) == _hx(st["v"]), tag + "v"
        assert m.d == _hx(st["d"]), tag + "d"
        assert (m.stepi, m.i, m.fev, m.ierr) == (float.fromhex(st["stepi"]), st["i"], st["fev"], st["ierr"]), tag + "scalars"

    m.init(guess)
    for _ in range(skip):
        m.iterate()
    same(rec["before"], name + " before ")
    m.paths = {k: 0 for k in rm.PATHS}
    out = {"name": name, "n": n, "objective": obj, "guess": [v.hex() for v in guess], "params": dict(par),
           "skip": skip, "before": {"state_crc": m.state_crcs(), "i": m.i, "fev": m.fev}, "states": []}
    assert len(rec["states"]) == WINDOW, name
    for g, st in enumerate(rec["states"]):
        m.evals = []
        i0 = m.i
        m.iterate()
        tag = "%s search %d " % (name, skip + g)
        assert flat_evals(m) == _hx(st["evals"]), tag + "evals"
        assert m.fs == _hx(st["fs"]), tag + "fs"
        same(st, tag)
        out["states"].append({"i0": i0, "i1": m.i, "fev": m.fev, "stepi": m.stepi.hex(), "di": m.d[i0].hex(),
                              "path": list(m.path), "orth": int(m.orth), "state_crc": m.state_crcs(),
                              "evals_crc": rm.crc(flat_evals(m)), "nevals": len(m.evals), "ok": bool(m.ok())})
    out["paths"] = dict(m.paths)
    return out


def record_steps(exe, shape):
    name, n, obj, base, step0 = shape
    par = dict(STEP_PARAMS, step0=step0)
    for attempt in range(STARTS_TRIED):
        guess = start_point(n, base, attempt)
        skip = window_start(shape, par, guess)
        if skip is None:
            continue
        out = replay_steps(call(exe, "steps", obj, n, par, skip, WINDOW, guess), shape, par, skip, guess)
        if sum(st["ok"] for st in out["states"]) >= GOOD_OK:
            return out
    sys.exit("%s: no start of %d with %d comparable searches" % (name, STARTS_TRIED, GOOD_OK))


def record_run(exe, shape):
    import rosenbrock_model as rm
    name, n, obj, base, mfev, tol, step0, decf = shape
    par = dict(mfev=mfev, tol=tol, step0=step0, decf=decf)
    guess = start_point(n, base)
    rec = call(exe, "run", obj, n, par, 0, 0, guess)
    m = model_of(obj, n, par)
    x, fev, conv = m.optimize(guess)
    assert flat_evals(m) == _hx(rec["evals"]), name + ": the points and values of the run"
    assert x == _hx(rec["x"]) and fev == rec["fev"] and int(conv) == rec["converged"], name + ": the result"
    return {"name": name, "n": n, "objective": obj, "guess": [v.hex() for v in guess], "params": par,
            "x": [v.hex() for v in x], "fev": fev, "converged": int(conv), "evals_crc": rm.crc(flat_evals(m)),
            "nevals": len(m.evals), "searches": m.searches, "orths": m.orths, "paths": dict(m.paths)}


def signature(ref):
    """the argument names and defaults of the constructor (rosenbrock.h:55)"""
    with open(os.path.join(ref, "src", "multivariate", "rosenbrock", "rosenbrock.h"), errors="replace") as fh:
        text = " ".join(fh.read().split())
    body = re.search(r"Rosenbrock\(([^)]*)\);", text).group(1)
    sig = []
    for arg in body.split(","):
        kind, name, default = re.match(r"\s*(\w+)\s+(\w+)\s*(?:=\s*([\w.+-]+))?\s*$", arg).groups()
        if default is None:
            sig.append({"name": name, "required": True})
        else:
            sig.append({"name": name, "required": False, "default": float(default) if kind == "double" else int(default)})
    return sig


def generate(ref="/root/reference"):
    import rosenbrock_model as rm
    tmp = tempfile.mkdtemp(prefix="rosenbrock_golden_")
    try:
        exe = build(ref, tmp)
        steps = [record_steps(exe, shape) for shape in STEP_SHAPES]
        runs = [record_run(exe, shape) for shape in RUN_SHAPES]
        have = {k: 0 for k in rm.PATHS}
        for rec in steps + runs:
            for k in rm.PATHS:
                have[k] += rec["paths"][k]
        for k in rm.PATHS:
            if have[k] < 2:
                sys.exit("path %s met %d times only (all: %s)" % (k, have[k], have))
        return {"steps": steps, "runs": runs, "paths": have, "signature": signature(ref)}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def time_reference(ref="/root/reference"):
    """us per line search of the reference on one core: the shapes of scripts/bench_rosenbrock.py"""
    tmp = tempfile.mkdtemp(prefix="rosenbrock_time_")
    try:
        exe = build(ref, tmp)
        par = dict(mfev=1 << 30, tol=0., step0=1., decf=0.1)
        for n, count in ((32, 20000), (128, 5000)):
            guess = start_point(n, -2.)
            runs = [call(exe, "time", "rosenbrock", n, par, 2 * n, count, guess) for _ in range(5)]
            us = sorted(r["us_per_search"] for r in runs)
            print("n = %d: %.3f us per line search (median of 5 runs of %d searches; least %.3f, largest %.3f)"
                  % (n, us[2], runs[0]["searches"], us[0], us[-1]))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def dumps(data):
    return json.dumps(data, sort_keys=True, separators=(",", ":")) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "rosenbrock_runs.json"))
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
    for rec in data["steps"]:
        print("%s: window from search %d, ok %d of %d, paths %s"
              % (rec["name"], rec["skip"], sum(s["ok"] for s in rec["states"]), len(rec["states"]),
                 {k: v for k, v in rec["paths"].items() if v}))
    for rec in data["runs"]:
        print("%s: %d evaluations, %d searches, %d orthogonalisations, converged %d, paths %s"
              % (rec["name"], rec["fev"], rec["searches"], rec["orths"], rec["converged"],
                 {k: v for k, v in rec["paths"].items() if v}))
    print("paths over the fixture: %s" % data["paths"])
    print("wrote %s (%d bytes)" % (a.out, len(text)))


if __name__ == "__main__":
    main()
