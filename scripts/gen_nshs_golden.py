#!/usr/bin/env python3
"""Records states of the REAL NSHS of the reference into tests/golden/nshs_runs.json (needs the
reference's sources and g++; run on the development machine, never where the GPU tests run).

    python scripts/gen_nshs_golden.py [--ref /root/reference] [--out tests/golden/nshs_runs.json]
    python scripts/gen_nshs_golden.py --time      # the reference's us per iteration, one core

A small harness (the C++ text below, this project's own) is compiled in a temporary directory
against the reference's nshs.cpp with the flags of oracle/Makefile (-O2 -ffp-contract=off).  It
seeds effolkronium::random_static::seed(k) and drives a subclass probe (the members of NSHS are
protected).

"steps": the state after init() and after each of the first 12 iterations: the memory, its values,
the candidate and its value, fstd, the rows of the best and of the worst (the first minimum and the
first maximum of the values, as std::min_element / std::max_element find them), it and fev; after
init the memory and its values are stored as the rows that changed (compress()).  Each
iteration also carries the raw 32-bit words it took from the global mt19937 -- exactly as many as
iterate() consumed, counted on a copy of the engine.  Six wide shapes (fstd > fstdmin = 1e-4 in
every recorded state) and four narrow ones (a small box and a large fstdmin: fstd <= fstdmin in
every state); the generator asserts the branch.  It also asserts that no decision is close: the
candidate's value against the worst and against the best it met, the worst against the second
worst, the best against the runner-up and fstd against fstdmin all differ by more than 1e-6
relative in every recorded state, so that no comparison against the fixture can turn on a flip; a
seed that fails is replaced.
"bands": the sorted final f(best) of 256 seeds (1000 + s) at a fixed budget on the sphere and on
Rosenbrock, n = 10, hms = 20.
"signature": the argument names and defaults of NSHS's constructor as bound at
py/multivariate_py.cpp:200-205.
Floats are float.hex strings.  The fixture holds numbers and names only.
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

# (name, n, hms, objective, box, fstdmin, seed)
SHAPES = [
    ("wide_n1_h3", 1, 3, "sphere", 4., 1e-4, 11),
    ("wide_n2_h5", 2, 5, "rosenbrock", 3., 1e-4, 22),
    ("wide_n3_h7", 3, 7, "ellipsoid", 5., 1e-4, 33),
    ("wide_n5_h20", 5, 20, "rosenbrock", 5., 1e-4, 44),
    ("wide_n9_h20", 9, 20, "sphere", 5., 1e-4, 55),
    ("wide_n17_h4", 17, 4, "ellipsoid", 5., 1e-4, 66),
    ("narrow_n2_h5", 2, 5, "sphere", 0.5, 0.25, 77),
    ("narrow_n3_h7", 3, 7, "sphere", 0.5, 0.4, 88),
    ("narrow_n5_h20", 5, 20, "sphere", 0.5, 0.5, 99),
    ("narrow_n9_h20", 9, 20, "sphere", 0.25, 0.25, 111),
]
ITERATIONS = 12
# one short record under the per-coordinate box of tests/_boxes.py (the harness is handed its bounds, box_arg):
# the fresh value, the bandwidth (up[i] - lo[i]) / tunerange and the clamp with bounds that differ in every coordinate
PERCOORD = ("percoord_n11_h6", 11, 6, "sphere", "percoord", 1e-4, 123)
PERCOORD_ITERATIONS = 5
MFEV = 1000000
MIN_GAP = 1e-6
OBJ_IDS = {"sphere": 0, "rosenbrock": 1, "rastrigin": 2, "ellipsoid": 3, "ackley": 4,
           "griewank": 5, "cigar": 6, "discus": 7, "diffpow": 8, "schwefel12": 9}
BANDS = dict(n=10, hms=20, mfev=4000, fstdmin=0.0001, box=5., seed0=1000, count=256)
SIGNATURE = [{"name": "mfev", "required": True}, {"name": "hms", "required": True},
             {"name": "fstdmin", "required": False, "default": 0.0001}]

HARNESS = r"""
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <random>
#include <string>
#include <vector>
#include "objectives.h"
#include "random.hpp"
#include "multivariate/multivariate.h"
#include "multivariate/harmony/nshs.h"

using Random = effolkronium::random_static;

struct Probe: public NSHS {
    using NSHS::NSHS;
    static void vec(const char *k, const std::vector<double> &v, bool last = false)
    {
        printf("\"%s\":[", k);
        for (size_t i = 0; i < v.size(); i++) printf("%s\"%a\"", i ? "," : "", v[i]);
        printf("]%s", last ? "" : ",");
    }
    void dump()
    {
        std::vector<double> x, f;
        for (auto &h : _hm) {
            x.insert(x.end(), h._x.begin(), h._x.end());
            f.push_back(h._f);
        }
        const int ibest = (int) (std::min_element(_hm.begin(), _hm.end(), harmony::compare_fitness) - _hm.begin());
        const int iworst = (int) (std::max_element(_hm.begin(), _hm.end(), harmony::compare_fitness) - _hm.begin());
        vec("x", x); vec("f", f); vec("cand", _temp._x);
        printf("\"fcand\":\"%a\",\"fstd\":\"%a\",\"ibest\":%d,\"ibest_kept\":%d,\"iworst\":%d,\"it\":%d,\"fev\":%d",
                _temp._f, _fstd, ibest, (int) (_best - &_hm[0]), iworst, _it, _fev);
    }
    double fbest() const { return _best->_f; }
};

struct Ctx { int obj, n; std::vector<double> aux; };

// "l0,l1,...|u0,u1,...": bounds given coordinate by coordinate (box_arg() below writes them from
// tests/_boxes.py); false, and nothing touched, where `s` is a plain number
static bool bounds_arg(const char *s, std::vector<double> &lo, std::vector<double> &up)
{
    if (!strchr(s, '|')) return false;
    std::vector<double> *v = &lo;
    size_t i = 0;
    for (const char *p = s; *p;) {
        if (*p == '|') { v = &up; i = 0; p++; continue; }
        if (*p == ',') { p++; continue; }
        char *e;
        const double x = strtod(p, &e);
        if (i < v->size()) (*v)[i++] = x;
        p = e;
    }
    return true;
}

int main(int argc, char **argv)
{
    // steps <obj> <n> <hms> <box> <seed> <iterations> <fstdmin> <mfev>
    // bands <obj> <n> <hms> <mfev> <fstdmin> <box> <seed0> <count>
    // time  <obj> <n> <hms> <iterations>
    Ctx c { atoi(argv[2]), atoi(argv[3]), {} };
    const int n = c.n;
    c.aux.resize(n);
    bbo_objective_aux(c.obj, n, c.aux.data());
    multivariate f = [&c](const double *x) { return bbo_objective_eval(c.obj, c.n, x, c.aux.data()); };
    if (!strcmp(argv[1], "steps")) {
        const double box = atof(argv[5]);
        std::vector<double> lo(n, -box), up(n, box), guess(n, 0.);
        bounds_arg(argv[5], lo, up);
        multivariate_problem prob { f, n, lo.data(), up.data() };
        Random::seed((unsigned) atoi(argv[6]));
        Probe p(atoi(argv[9]), atoi(argv[4]), atof(argv[8]));
        p.init(prob, guess.data());
        printf("{\"init\":{");
        p.dump();
        printf("},\"states\":[");
        const int its = atoi(argv[7]);
        for (int g = 1; g <= its; g++) {
            auto before = Random::get_engine();
            p.iterate();
            const auto after = Random::get_engine();
            printf("%s{\"words\":[", g > 1 ? "," : "");
            for (int i = 0; !(before == after); i++) printf("%s%u", i ? "," : "", (unsigned) before());
            printf("],");
            p.dump();
            printf("}");
        }
        printf("]}\n");
    } else if (!strcmp(argv[1], "bands")) {
        const double box = atof(argv[7]);
        std::vector<double> lo(n, -box), up(n, box), guess(n, 0.);
        multivariate_problem prob { f, n, lo.data(), up.data() };
        const int seed0 = atoi(argv[8]), count = atoi(argv[9]);
        std::vector<double> out;
        for (int s = 0; s < count; s++) {
            Random::seed((unsigned) (seed0 + s));
            Probe p(atoi(argv[5]), atoi(argv[4]), atof(argv[6]));
            p.optimize(prob, guess.data());
            out.push_back(p.fbest());
        }
        printf("{");
        Probe::vec("fbest", out, true);
        printf("}\n");
    } else {
        std::vector<double> lo(n, -5.), up(n, 5.), guess(n, 0.);
        multivariate_problem prob { f, n, lo.data(), up.data() };
        Random::seed(1u);
        const int its = atoi(argv[5]);
        Probe p(atoi(argv[4]) + 2 * its + 100, atoi(argv[4]), 0.0001);
        p.init(prob, guess.data());
        for (int g = 0; g < 100; g++) p.iterate();
        const auto t0 = std::chrono::steady_clock::now();
        for (int g = 0; g < its; g++) p.iterate();
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        printf("{\"us_per_iteration\":%.6f}\n", us / its);
    }
    return 0;
}
"""


def _norm(obj):
    """hex strings as Python writes them (the C library's %a may choose another normalisation)"""
    if isinstance(obj, dict):
        return {k: _norm(v) for k, v in obj.items()}
    if isinstance(obj, list):
        return [_norm(v) for v in obj]
    if isinstance(obj, str) and ("0x" in obj or obj in ("inf", "-inf", "nan", "-nan")):
        return float.fromhex(obj).hex() if "0x" in obj else float(obj.replace("-nan", "nan")).hex()
    return obj


def build(ref, tmp):
    src = os.path.join(ref, "src")
    with open(os.path.join(tmp, "harness.cpp"), "w") as fh:
        fh.write(HARNESS)
    exe = os.path.join(tmp, "harness")
    subprocess.check_call(
        ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-w", "-include", "cmath", "-I" + src,
         "-I" + os.path.join(ROOT, "oracle"), "-o", exe, os.path.join(tmp, "harness.cpp"),
         os.path.join(src, "multivariate/harmony/nshs.cpp"), "-lm"])
    return exe


def _far(a, b):
    return abs(a - b) > MIN_GAP * max(abs(a), abs(b))


def checks(rec, fstdmin, wide):
    """the branch in every recorded state, and no close decision (see the module's text)"""
    prev = rec["init"]
    states = [rec["init"]] + rec["states"]
    for st in states:
        f = sorted(float.fromhex(v) for v in st["f"])
        fstd = float.fromhex(st["fstd"])
        if (fstd > fstdmin) != wide or not _far(fstd, fstdmin):
            return False
        if len(f) > 1 and not (_far(f[0], f[1]) and _far(f[-1], f[-2])):
            return False
        if st["ibest"] != st["ibest_kept"]:
            return False
    for st in rec["states"]:
        f = [float.fromhex(v) for v in prev["f"]]
        fc = float.fromhex(st["fcand"])
        if not (_far(fc, max(f)) and _far(fc, min(f))):
            return False
        prev = st
    return True


def compress(rec, n):
    """an iteration changes one row at most: after init a state keeps the rows of the memory and the
    values that differ from the state before it, as {row: ...} under "x_rows" and "f_rows"
    (tests/test_nshs_model.py puts the whole memory back)"""
    x, f = rec["init"]["x"], rec["init"]["f"]
    for st in rec["states"]:
        nx, nf = st.pop("x"), st.pop("f")
        st["x_rows"] = {str(i): nx[i * n:(i + 1) * n] for i in range(len(nf)) if nx[i * n:(i + 1) * n] != x[i * n:(i + 1) * n]}
        st["f_rows"] = {str(i): nf[i] for i in range(len(nf)) if nf[i] != f[i]}
        x, f = nx, nf


def box_arg(box, n):
    """the harness's box argument: a number, or for "percoord" the bounds of tests/_boxes.py, "l0,..|u0,.." """
    if box != "percoord":
        return repr(box)
    from _boxes import percoord_box
    lo, up = percoord_box(n)
    return ",".join(repr(float(v)) for v in lo) + "|" + ",".join(repr(float(v)) for v in up)


def record(exe, name, n, hms, obj, box, fstdmin, seed, iterations=ITERATIONS, wide=None):
    """one shape; the seed moves on until the branch holds and no decision is close (`wide`: the branch,
    where the name does not begin with it)"""
    wide = name.startswith("wide") if wide is None else wide
    for attempt in range(64):
        out = subprocess.check_output(
            [exe, "steps", str(OBJ_IDS[obj]), str(n), str(hms), box_arg(box, n), str(seed + 1000 * attempt),
             str(iterations), repr(fstdmin), str(MFEV)])
        rec = _norm(json.loads(out))
        if checks(rec, fstdmin, wide):
            break
    else:
        sys.exit("%s: no seed that keeps its branch without a close decision" % name)
    assert checks(rec, fstdmin, wide), name
    for st in [rec["init"]] + rec["states"]:
        del st["ibest_kept"]
    replaced = sum(a["f"] != b["f"] for a, b in zip([rec["init"]] + rec["states"], rec["states"]))
    compress(rec, n)
    rec.update({"name": name, "n": n, "hms": hms, "objective": obj, "box": box,
                "fstdmin": fstdmin, "mfev": MFEV, "wide": wide, "seed": seed + 1000 * attempt, "replacements": replaced})
    return rec


def generate_percoord(ref="/root/reference"):
    """tests/golden/nshs_percoord.json: PERCOORD alone"""
    tmp = tempfile.mkdtemp(prefix="nshs_golden_")
    try:
        return {"steps": [record(build(ref, tmp), *PERCOORD, iterations=PERCOORD_ITERATIONS, wide=True)]}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def generate(ref="/root/reference"):
    tmp = tempfile.mkdtemp(prefix="nshs_golden_")
    try:
        exe = build(ref, tmp)
        steps = [record(exe, *shape) for shape in SHAPES]
        bands = dict(BANDS)
        b = BANDS
        for obj in ("sphere", "rosenbrock"):
            out = subprocess.check_output(
                [exe, "bands", str(OBJ_IDS[obj]), str(b["n"]), str(b["hms"]), str(b["mfev"]), repr(b["fstdmin"]),
                 repr(b["box"]), str(b["seed0"]), str(b["count"])])
            vals = sorted(float.fromhex(v) for v in json.loads(out)["fbest"])
            bands[obj] = [v.hex() for v in vals]
        return {"steps": steps, "bands": bands, "signature": SIGNATURE}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def time_reference(ref="/root/reference"):
    """us per iteration of the reference on one core: the shape of scripts/bench_nshs.py"""
    tmp = tempfile.mkdtemp(prefix="nshs_time_")
    try:
        exe = build(ref, tmp)
        for n, hms, its in ((128, 20, 200000),):
            best = min(json.loads(subprocess.check_output(
                [exe, "time", str(OBJ_IDS["rosenbrock"]), str(n), str(hms), str(its)]))["us_per_iteration"]
                for _ in range(5))
            print("n = %d, hms = %d: %.3f us per iteration (best of 5 runs of %d)" % (n, hms, best, its))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def dumps(data):
    return json.dumps(data, sort_keys=True, separators=(",", ":")) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "nshs_runs.json"))
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--percoord", action="store_true",
                    help="write the per-coordinate record alone, to tests/golden/nshs_percoord.json")
    a = ap.parse_args()
    if not os.path.isdir(os.path.join(a.ref, "src")):
        sys.exit("the reference sources are not at %s" % a.ref)
    if a.time:
        time_reference(a.ref)
        return
    if a.percoord and a.out.endswith("nshs_runs.json"):
        a.out = os.path.join(ROOT, "tests", "golden", "nshs_percoord.json")
    data = generate_percoord(a.ref) if a.percoord else generate(a.ref)
    text = dumps(data)
    with open(a.out, "w") as fh:
        fh.write(text)
    for rec in data["steps"]:
        print("%s: seed %d, %d replacements" % (rec["name"], rec["seed"], rec["replacements"]))
    print("wrote %s (%d bytes)" % (a.out, len(text)))


if __name__ == "__main__":
    main()
