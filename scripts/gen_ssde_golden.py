#!/usr/bin/env python3
"""Records states of the REAL SSDE of the reference into tests/golden/ssde_runs.json (needs the reference's
sources and g++; run on the development machine, never where the GPU tests run).

    python scripts/gen_ssde_golden.py [--ref /root/reference] [--out tests/golden/ssde_runs.json]
    python scripts/gen_ssde_golden.py --time      # the reference's ms per generation, one core

A small harness (the C++ text below, this project's own) is compiled in a temporary directory against the
reference's ssde.cpp and blas.cpp with the flags of oracle/Makefile (-O2 -ffp-contract=off).  It seeds
effolkronium::random_static::seed(k) and drives a subclass probe (the members of SSDESearch are protected).

"steps": the state after init() and after each of the first GENERATIONS calls of iterate(): x f (the pool
in its sorted order) L1 L2 LCR k kCR np fev convcount perm, and every point the generation handed to the
objective with its value ("pts", "vals").  The harness also prints the raw 32-bit words each call took from
the global mt19937 -- exactly as many as it consumed, counted on a copy of the engine.  They are the outputs
of std::mt19937 under the record's seed, so the fixture keeps their number and CRC-32 per generation, and
the float arrays of a state as the entries that changed since the state before (ssde_model.pack_states).

The generator replays every record through tests/ssde_model.py and fails unless the model reproduces every
state and every evaluated point bit for bit.  The seed of a shape moves on until, over the recorded
generations, no two stored values and no trial and the value it is compared with lie within MIN_GAP
relative, and no rejection loop (sample3, the Cauchy step) took more than MAX_ATTEMPTS draws.  The gap rule
is waived for n <= 2: a pool of four or five points in one or two dimensions is clamped onto the walls of
the box again and again, so no seed is free of equal values, and the one-term objectives there give the
same bits on every machine, so a close comparison is decided alike everywhere (equal values keep their
order on both sides: std::sort is an insertion sort below 16 elements).

"runs": fev, converged and x* of 64 complete optimize() runs (n = 4, npinit = 10, sphere and Rosenbrock,
usede both ways; the box is not symmetric about 0: with usede the pool starts as points and their opposites
lower + upper - x, which on a symmetric box have equal values in pairs under an even objective, and the
order std::sort leaves 2 npinit > 16 such values in is its own).  "bands": the sorted final best values of 256 seeds at a fixed budget, sphere and
Rosenbrock, n = 10, npinit = 50, usede both ways.  "signature": the argument names and defaults of SSDE's
constructor as bound in py/multivariate_py.cpp.  Single floats are float.hex strings, arrays packed doubles
in base64.  The fixture holds numbers and names only.
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

# name, n, npinit, objective, box, mfev, options, seed
SHAPES = [
    ("n1_np4", 1, 4, "sphere", (-5., 5.), 400, {}, 11),
    ("n2_np5", 2, 5, "rosenbrock", (-3., 3.), 500, {}, 22),
    ("n3_np6", 3, 6, "sphere", (-5., 5.), 240, {}, 33),
    ("n5_np20_de_h3", 5, 20, "rosenbrock", (-3., 3.), 190, {"usede": 1, "h": 3}, 44),
    ("n17_np20_de_norepair", 17, 20, "ellipsoid", (-3., 5.), 400, {"usede": 1, "repaircr": 0}, 55),
    ("n66_np8", 66, 8, "rosenbrock", (-3., 3.), 640, {}, 66),
]
GENERATIONS = 6
# one short record under the per-coordinate box of tests/_boxes.py (the harness is handed its bounds, box_arg): the
# opposition point lower + upper - x of the usede start and the redraw, with bounds that differ in every coordinate
PERCOORD = ("percoord_n11_np12_de", 11, 12, "sphere", "percoord", 400, {"usede": 1}, 77)
PERCOORD_GENERATIONS = 5
TOL = 1e-12
MIN_GAP = 1e-6
MAX_ATTEMPTS = 8
EXACT_N = 2     # up to here the objective is one term: every value is bit-exact on any machine
DEFAULTS = {"patience": 1000, "npmin": 4, "ptop": 0.11, "h": 100, "usede": 0, "repaircr": 1}
OBJ_IDS = {"sphere": 0, "rosenbrock": 1, "rastrigin": 2, "ellipsoid": 3, "ackley": 4,
           "griewank": 5, "cigar": 6, "discus": 7, "diffpow": 8, "schwefel12": 9}
RUNS = dict(n=4, npinit=10, mfev=600, tol=1e-3, box=(-5., 7.), seed0=3000, count=16)
BANDS = dict(n=10, npinit=50, mfev=1500, tol=0., box=(-5., 5.), seed0=7000, count=256)
SIGNATURE = [{"name": "mfev", "required": True}, {"name": "npinit", "required": True},
             {"name": "tol", "required": True},
             {"name": "patience", "required": False, "default": 1000},
             {"name": "npmin", "required": False, "default": 4},
             {"name": "ptop", "required": False, "default": 0.11},
             {"name": "h", "required": False, "default": 100},
             {"name": "usede", "required": False, "default": False},
             {"name": "repaircr", "required": False, "default": True}]

HARNESS = r"""
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <random>
#include <vector>
#include "objectives.h"
#include "random.hpp"
#include "multivariate/multivariate.h"
#include "multivariate/de/ssde.h"

using Random = effolkronium::random_static;

static void vec(const char *k, const std::vector<double> &v)
{
    printf("\"%s\":[", k);
    for (size_t i = 0; i < v.size(); i++) printf("%s\"%a\"", i ? "," : "", v[i]);
    printf("],");
}

struct Probe: public SSDESearch {
    using SSDESearch::SSDESearch;
    void dump()
    {
        std::vector<double> x, f;
        for (auto &k : _swarm) {
            x.insert(x.end(), k._x.begin(), k._x.end());
            f.push_back(k._f);
        }
        vec("x", x); vec("f", f); vec("L1", _L1); vec("L2", _L2); vec("LCR", _LCR);
        printf("\"perm\":[");
        for (size_t i = 0; i < _iwork.size(); i++) printf("%s%d", i ? "," : "", _iwork[i]);
        printf("],\"k\":%d,\"kCR\":%d,\"np\":%d,\"fev\":%d,\"convcount\":%d", _k, _kCR, _np, _fev, _convcount);
    }
    double fbest() const { return _swarm[0]._f; }
};

struct Ctx { int obj, n; std::vector<double> aux, pts, vals; bool log; };

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
    // steps <obj> <n> <npinit> <lo> <up> <seed> <generations> <mfev> <tol> <patience> <npmin> <ptop> <h> <usede> <repaircr>
    // runs  <obj> <n> <npinit> <lo> <up> <seed0> <count> <mfev> <tol> <usede>
    // time  <obj> <n> <npinit> <generations> <usede>
    Ctx c { atoi(argv[2]), atoi(argv[3]), {}, {}, {}, false };
    const int n = c.n, npinit = atoi(argv[4]);
    c.aux.resize(n);
    bbo_objective_aux(c.obj, n, c.aux.data());
    multivariate f = [&c](const double *x) {
        const double v = bbo_objective_eval(c.obj, c.n, x, c.aux.data());
        if (c.log) {
            c.pts.insert(c.pts.end(), x, x + c.n);
            c.vals.push_back(v);
        }
        return v;
    };
    if (!strcmp(argv[1], "steps")) {
        std::vector<double> lo(n, atof(argv[5])), up(n, atof(argv[6])), guess(n, 0.);
        bounds_arg(argv[5], lo, up);
        multivariate_problem prob { f, n, lo.data(), up.data() };
        Random::seed((unsigned) atoi(argv[7]));
        Probe p(atoi(argv[9]), npinit, atof(argv[10]), atoi(argv[11]), atoi(argv[12]), atof(argv[13]), atoi(argv[14]),
                atoi(argv[15]) != 0, atoi(argv[16]) != 0);
        auto start = Random::get_engine();
        p.init(prob, guess.data());
        const auto inited = Random::get_engine();
        int init_words = 0;
        for (; !(start == inited); init_words++) start();
        printf("{\"init\":{\"words\":%d,", init_words);
        p.dump();
        printf("},\"states\":[");
        const int gens = atoi(argv[8]);
        c.log = true;
        for (int g = 1; g <= gens; g++) {
            auto before = Random::get_engine();
            c.pts.clear();
            c.vals.clear();
            p.iterate();
            const auto after = Random::get_engine();
            printf("%s{\"words\":[", g > 1 ? "," : "");
            for (int i = 0; !(before == after); i++) printf("%s%u", i ? "," : "", (unsigned) before());
            printf("],");
            vec("pts", c.pts);
            vec("vals", c.vals);
            p.dump();
            printf("}");
        }
        printf("]}\n");
    } else if (!strcmp(argv[1], "runs")) {
        std::vector<double> lo(n, atof(argv[5])), up(n, atof(argv[6])), guess(n, 0.);
        multivariate_problem prob { f, n, lo.data(), up.data() };
        const int seed0 = atoi(argv[7]), count = atoi(argv[8]);
        printf("[");
        for (int s = 0; s < count; s++) {
            Random::seed((unsigned) (seed0 + s));
            Probe p(atoi(argv[9]), npinit, atof(argv[10]), 1000, 4, 0.11, 100, atoi(argv[11]) != 0, true);
            const auto sol = p.optimize(prob, guess.data());
            printf("%s{\"seed\":%d,\"fev\":%d,\"converged\":%d,\"fbest\":\"%a\",", s ? "," : "", seed0 + s,
                    sol._fev, sol._converged ? 1 : 0, p.fbest());
            vec("x", sol._sol);
            printf("\"n\":%d}", n);
        }
        printf("]\n");
    } else {
        std::vector<double> lo(n, -5.), up(n, 5.), guess(n, 0.);
        multivariate_problem prob { f, n, lo.data(), up.data() };
        Random::seed(1u);
        const int gens = atoi(argv[5]);
        Probe p(100 * npinit * (gens + 20), npinit, 0., 1000000, npinit, 0.11, 100, atoi(argv[6]) != 0, true);
        p.init(prob, guess.data());
        for (int g = 0; g < 20; g++) p.iterate();
        const int fev0 = p.solution()._fev;
        const auto t0 = std::chrono::steady_clock::now();
        for (int g = 0; g < gens; g++) p.iterate();
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        printf("{\"ms_per_generation\":%.6f,\"evals_per_generation\":%.3f}\n", ms / gens,
                (double) (p.solution()._fev - fev0) / gens);
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
         os.path.join(src, "multivariate/de/ssde.cpp"), os.path.join(src, "blas.cpp"), "-lm"])
    return exe


def options(rec):
    return {k: rec.get(k, v) for k, v in DEFAULTS.items()}


def model_of(rec, f=None, min_np=0):
    import chol_model
    import ssde_model as sm
    n, o = rec["n"], options(rec)
    lo, up = sm.box_of(rec)
    return sm.Ssde(f or chol_model.objective(rec["objective"], n), lo, up, rec["mfev"],
                   rec["npinit"], rec["tol"], o["patience"], o["npmin"], o["ptop"], o["h"], bool(o["usede"]),
                   bool(o["repaircr"]), min_np=min_np)


def replay(rec):
    """the raw record through tests/ssde_model.py: (reproduced bit for bit, events, smallest gap, attempts)"""
    import numpy as np
    import jaya_model as jm
    import ssde_model as sm

    def h(v):
        return np.array([float.fromhex(s) for s in v])

    n, npinit = rec["n"], rec["npinit"]
    m = model_of(rec)
    m.trace = True
    m.start(h(rec["init"]["x"]).reshape(npinit, n), h(rec["init"]["f"]), fev=rec["init"]["fev"])
    m.gaps = []
    for a, b in zip(m.fx, m.fx[1:]):
        m._gap(a, b)
    have, saved, attempts = False, 0., 0
    for st in rec["states"]:
        w = jm.Words(st["words"])
        w.have, w.saved = have, saved
        src = sm.WordsSource(w, n, npinit)
        m.points = []
        m.iterate(src)
        have, saved = w.have, w.saved
        attempts = max(attempts, src.attempts)
        if not w.exhausted():
            return False, set(), 0., 0
        got = m.state()
        for k in sm.Ssde.KEYS:
            want = st[k]
            if k in sm.FLOAT_KEYS:
                if np.asarray(got[k], float).tobytes() != h(want).tobytes():
                    return False, set(), 0., 0
            elif k == "perm":
                if list(got[k]) != list(want):
                    return False, set(), 0., 0
            elif int(got[k]) != want:
                return False, set(), 0., 0
        pts = np.array([v for p, _ in m.points for v in p])
        vals = np.array([v for _, v in m.points])
        if pts.tobytes() != h(st["pts"]).tobytes() or vals.tobytes() != h(st["vals"]).tobytes():
            return False, set(), 0., 0
    rec["repairs"] = dict(m.repairs)
    return True, set(m.events), min(m.gaps) if m.gaps else 1., attempts


def box_arg(box, n):
    """the harness's box argument: a number, or for "percoord" the bounds of tests/_boxes.py, "l0,..|u0,.." """
    if box != "percoord":
        return repr(box)
    from _boxes import percoord_box
    lo, up = percoord_box(n)
    return ",".join(repr(float(v)) for v in lo) + "|" + ",".join(repr(float(v)) for v in up)


def box_args(box, n):
    """the harness's two box arguments: lower and upper, or the bounds string and a placeholder"""
    return [box_arg(box, n), "0"] if box == "percoord" else [repr(box[0]), repr(box[1])]


def record(exe, name, n, npinit, obj, box, mfev, opts, seed, generations=GENERATIONS, need_repairs=0):
    o = dict(DEFAULTS)
    o.update(opts)
    for attempt in range(400):
        out = subprocess.check_output(
            [exe, "steps", str(OBJ_IDS[obj]), str(n), str(npinit), *box_args(box, n), str(seed + 1000 * attempt),
             str(generations), str(mfev), repr(TOL), str(o["patience"]), str(o["npmin"]), repr(o["ptop"]),
             str(o["h"]), str(o["usede"]), str(o["repaircr"])])
        rec = _norm(json.loads(out))
        rec.update({"name": name, "n": n, "npinit": npinit, "objective": obj,
                    "box": box if box == "percoord" else list(box), "mfev": mfev, "tol": TOL,
                    "seed": seed + 1000 * attempt})
        rec.update(opts)
        same, events, gap, attempts = replay(rec)
        if not same:
            sys.exit("%s: tests/ssde_model.py does not reproduce the reference (seed %d)" % (name, rec["seed"]))
        if (gap >= MIN_GAP or n <= EXACT_N) and attempts <= MAX_ATTEMPTS \
                and min(rec["repairs"].values()) >= need_repairs:
            break
    else:
        sys.exit("%s: no seed without a close decision" % name)
    rec["events"] = sorted(events)
    rec["min_gap"] = gap
    rec["max_attempts"] = attempts
    compact(rec)
    return rec


def compact(rec):
    """the record in the fixture's form: per generation the number and CRC-32 of its words (after checking
    that ssde_model.Mt19937Words makes exactly the recorded words from the seed), float arrays packed"""
    import ssde_model as sm
    live = sm.Mt19937Words(rec["seed"])
    live.take(rec["init"]["words"])
    for st in rec["states"]:
        words = st["words"]
        if live.take(len(words)) != words:
            sys.exit("%s: the seed does not give back the recorded words" % rec["name"])
        st["words"] = {"count": len(words), "crc32": sm.words_crc(words)}
        st["pts"] = sm.b64([float.fromhex(v) for v in st["pts"]])
        st["vals"] = sm.b64([float.fromhex(v) for v in st["vals"]])
    states = [rec["init"]] + rec["states"]
    for st in states:
        for k in sm.FLOAT_KEYS:
            st[k] = [float.fromhex(v) for v in st[k]]
    sm.pack_states(states)


def runs_of(exe, obj, b, usede, seed0=None, count=None):
    out = subprocess.check_output(
        [exe, "runs", str(OBJ_IDS[obj]), str(b["n"]), str(b["npinit"]), repr(b["box"][0]), repr(b["box"][1]),
         str(b["seed0"] if seed0 is None else seed0), str(b["count"] if count is None else count), str(b["mfev"]),
         repr(b["tol"]), str(usede)])
    return _norm(json.loads(out))


def generate(ref="/root/reference"):
    tmp = tempfile.mkdtemp(prefix="ssde_golden_")
    try:
        exe = build(ref, tmp)
        steps = [record(exe, *shape) for shape in SHAPES]
        seen = set().union(*(set(r["events"]) for r in steps))
        wanted = {"explore", "balance", "exploit", "ss_success", "de_success", "de_failure", "wrap", "shrink"}
        if not wanted <= seen:
            sys.exit("the steps runs never take: %s" % sorted(wanted - seen))
        runs, bands = dict(RUNS), dict(BANDS)
        runs["cases"] = []
        for obj in ("sphere", "rosenbrock"):
            for usede in (0, 1):
                for r in runs_of(exe, obj, RUNS, usede):
                    r.update({"objective": obj, "usede": usede})
                    runs["cases"].append(r)
                vals = sorted(float.fromhex(r["fbest"]) for r in runs_of(exe, obj, BANDS, usede))
                bands["%s_usede%d" % (obj, usede)] = [v.hex() for v in vals]
        return {"steps": steps, "runs": runs, "bands": bands, "signature": SIGNATURE}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def generate_percoord(ref="/root/reference"):
    """tests/golden/ssde_percoord.json: PERCOORD alone, with at least three coordinates redrawn at each bound ("repairs")"""
    tmp = tempfile.mkdtemp(prefix="ssde_golden_")
    try:
        rec = record(build(ref, tmp), *PERCOORD, generations=PERCOORD_GENERATIONS, need_repairs=3)
        return {"steps": [rec]}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def time_reference(ref="/root/reference"):
    """ms per generation of the reference on one core: the shape of scripts/bench_ssde.py"""
    tmp = tempfile.mkdtemp(prefix="ssde_time_")
    try:
        exe = build(ref, tmp)
        for n, npinit, gens in ((128, 100, 200),):
            for usede in (0, 1):
                runs = [json.loads(subprocess.check_output(
                    [exe, "time", str(OBJ_IDS["rosenbrock"]), str(n), str(npinit), str(gens), str(usede)]))
                    for _ in range(5)]
                ms = sorted(r["ms_per_generation"] for r in runs)
                print("n = %d, npinit = %d, usede = %d: %.4f ms per generation (median of 5 runs of %d; min %.4f, "
                      "max %.4f), %.1f evaluations per generation"
                      % (n, npinit, usede, ms[2], gens, ms[0], ms[-1], runs[0]["evals_per_generation"]))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def dumps(data):
    return json.dumps(data, sort_keys=True, separators=(",", ":")) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ssde_runs.json"))
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--percoord", action="store_true",
                    help="write the per-coordinate record alone, to tests/golden/ssde_percoord.json")
    a = ap.parse_args()
    if not os.path.isdir(os.path.join(a.ref, "src")):
        sys.exit("the reference sources are not at %s" % a.ref)
    if a.time:
        time_reference(a.ref)
        return
    if a.percoord and a.out.endswith("ssde_runs.json"):
        a.out = os.path.join(ROOT, "tests", "golden", "ssde_percoord.json")
    data = generate_percoord(a.ref) if a.percoord else generate(a.ref)
    text = dumps(data)
    with open(a.out, "w") as fh:
        fh.write(text)
    for rec in data["steps"]:
        print("%s: seed %d, smallest gap %.2e, %d attempts, %s"
              % (rec["name"], rec["seed"], rec["min_gap"], rec["max_attempts"], " ".join(rec["events"])))
    print("wrote %s (%d bytes)" % (a.out, len(text)))


if __name__ == "__main__":
    main()
