#!/usr/bin/env python3
"""Records states of the REAL SLPSO of the reference into tests/golden/slpso_runs.json (needs the
reference's sources and g++; run on the development machine, never where the GPU tests run).

    python scripts/gen_slpso_golden.py [--ref /root/reference] [--out tests/golden/slpso_runs.json]
    python scripts/gen_slpso_golden.py --time      # the reference's ms per generation, one core

A small harness (the C++ text below, this project's own) is compiled in a temporary directory
against the reference's slpso.cpp and blas.cpp with the flags of oracle/Makefile (-O2
-ffp-contract=off).  It seeds effolkronium::random_static::seed(k) and drives a subclass probe (the
members of SLPSOSearch are protected).

"steps": the state after init() and after each of the first GENERATIONS calls of iterate(): x v pb fx
fpb fp s p g G m CF PF Uf Pl perm abest fabest vdavg alpha omega mfes fev.  The harness also prints the
raw 32-bit words each call took from the global mt19937 -- exactly as many as it consumed, counted on a
copy of the engine.  They are the outputs of std::mt19937 under the record's seed, so the fixture keeps
their number and CRC-32 per generation, and the float arrays as the entries that changed since the state
before (compact() below; tests/test_slpso_model.py puts words and arrays back).  The optimizer's normal distribution keeps its cached second value
across generations: a reader decodes one run with ONE jaya_model.Words state (tests/test_slpso_model.py
carries `have` / `saved` over).

The generator replays every record through tests/slpso_model.py and fails unless the model reproduces
every state bit for bit.  From the replay it also asserts that over all steps runs together all four
operators, the forced convergence operator, both branches of operator 2, the eq. 11 redraw on both
walls, an accepted and a rejected Algorithm 2 trial, a selection-ratio refresh and both CF / PF
transitions of Algorithm 3 occur.  The seed of a run moves on until every fitness comparison the
reference made in the record (fx<fp, fx<fpb, fx<fabest, fnew<fabest, j.fpb<k.fpb) has a relative gap
of at least MIN_GAP -- comparisons between the values of bit-identical points are exempt, the
first-generation operator 1 makes such points -- and until np (1 - exp(-100 pfev^3)) is not within
MIN_GAP of an integer (a saturated pfev = 1 gives np exactly on every platform and is exempt).

"runs": fev, converged and fabest of complete optimize() runs, 32 seeds each on the sphere and on
Rosenbrock, n = 10 in the box +-5, np = 20, stol = 1e-6, mfev = 40000.
"signature": the argument names and defaults of SLPSO's constructor as bound at
py/multivariate_py.cpp:292-299.
Single floats are float.hex strings, arrays packed doubles in base64.  The fixture holds numbers and names
only.
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

# (name, n, np, objective, box, Ufmax, seed)
SHAPES = [
    ("n2_np2", 2, 2, "rosenbrock", 3., 10., 11),
    ("n5_np3", 5, 3, "rosenbrock", 3., 10., 22),
    ("n12_np8_uf1", 12, 8, "ellipsoid", 5., 1., 33),
    ("n33_np6", 33, 6, "rosenbrock", 3., 10., 44),
    ("n65_np4", 65, 4, "sphere", 5., 10., 55),
]
GENERATIONS = 8
# one short record under the per-coordinate box of tests/_boxes.py (the harness is handed its bounds, box_arg): the
# eq. 11 redraw between a wall and the old position, and vmax, with bounds that differ in every coordinate
PERCOORD = ("percoord_n11_np6", 11, 6, "sphere", "percoord", 10., 66)
PERCOORD_GENERATIONS = 5
STOL = 1e-12
MIN_GAP = 1e-9
OBJ_IDS = {"sphere": 0, "rosenbrock": 1, "rastrigin": 2, "ellipsoid": 3, "ackley": 4,
           "griewank": 5, "cigar": 6, "discus": 7, "diffpow": 8, "schwefel12": 9}
RUNS = dict(n=10, np=20, mfev=40000, stol=1e-6, box=5., seed0=2000, count=32)
WANTED = {"op0", "op1", "op2", "op3", "forced", "op2_self", "op2_partner", "redraw_low", "redraw_high",
          "alg2_accept", "alg2_reject", "refresh", "cf_on", "cf_off"}
SIGNATURE = [{"name": "mfev", "required": True}, {"name": "stol", "required": True},
             {"name": "np", "required": True},
             {"name": "omegamin", "required": False, "default": 0.4},
             {"name": "omegamax", "required": False, "default": 0.9},
             {"name": "eta", "required": False, "default": 1.496},
             {"name": "gamma", "required": False, "default": 0.01},
             {"name": "vmax", "required": False, "default": 0.2},
             {"name": "Ufmax", "required": False, "default": 10.0}]

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
#include "multivariate/pso/slpso.h"

using Random = effolkronium::random_static;

struct Probe: public SLPSOSearch {
    using SLPSOSearch::SLPSOSearch;
    static void vec(const char *k, const std::vector<double> &v)
    {
        printf("\"%s\":[", k);
        for (size_t i = 0; i < v.size(); i++) printf("%s\"%a\"", i ? "," : "", v[i]);
        printf("],");
    }
    static void ints(const char *k, const std::vector<int> &v)
    {
        printf("\"%s\":[", k);
        for (size_t i = 0; i < v.size(); i++) printf("%s%d", i ? "," : "", v[i]);
        printf("],");
    }
    void dump()
    {
        std::vector<double> x, v, pb, fx, fpb, fp, s, p, Uf, Pl;
        std::vector<int> g, G, m, CF, PF;
        for (auto &k : _swarm) {
            x.insert(x.end(), k._x.begin(), k._x.end());
            v.insert(v.end(), k._v.begin(), k._v.end());
            pb.insert(pb.end(), k._pb.begin(), k._pb.end());
            fx.push_back(k._fx); fpb.push_back(k._fpb); fp.push_back(k._fp);
            s.insert(s.end(), k._s.begin(), k._s.end());
            p.insert(p.end(), k._p.begin(), k._p.end());
            g.insert(g.end(), k._g.begin(), k._g.end());
            G.insert(G.end(), k._G.begin(), k._G.end());
            m.push_back(k._m); CF.push_back(k._CF ? 1 : 0); PF.push_back(k._PF ? 1 : 0);
            Uf.push_back(k._Uf); Pl.push_back(k._Pl);
        }
        vec("x", x); vec("v", v); vec("pb", pb); vec("fx", fx); vec("fpb", fpb); vec("fp", fp);
        vec("s", s); vec("p", p); ints("g", g); ints("G", G); ints("m", m); ints("CF", CF); ints("PF", PF);
        vec("Uf", Uf); vec("Pl", Pl); ints("perm", _perm); vec("abest", _abest); vec("vdavg", _vdavg);
        printf("\"fabest\":\"%a\",\"alpha\":\"%a\",\"omega\":\"%a\",\"mfes\":%d,\"fev\":%d",
                _fabest, _alpha, _omega, _mfes, _fev);
    }
    double fabest() const { return _fabest; }
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
    // steps <obj> <n> <np> <box> <seed> <generations> <Ufmax> <mfev> <stol>
    // runs  <obj> <n> <np> <box> <seed0> <count> <mfev> <stol>
    // time  <obj> <n> <np> <generations>
    Ctx c { atoi(argv[2]), atoi(argv[3]), {} };
    const int n = c.n, np = atoi(argv[4]);
    c.aux.resize(n);
    bbo_objective_aux(c.obj, n, c.aux.data());
    multivariate f = [&c](const double *x) { return bbo_objective_eval(c.obj, c.n, x, c.aux.data()); };
    if (!strcmp(argv[1], "steps")) {
        const double box = atof(argv[5]);
        std::vector<double> lo(n, -box), up(n, box), guess(n, 0.);
        bounds_arg(argv[5], lo, up);
        multivariate_problem prob { f, n, lo.data(), up.data() };
        Random::seed((unsigned) atoi(argv[6]));
        Probe p(atoi(argv[9]), atof(argv[10]), np, 0.4, 0.9, 1.496, 0.01, 0.2, atof(argv[8]));
        auto start = Random::get_engine();
        p.init(prob, guess.data());
        const auto inited = Random::get_engine();
        int init_words = 0;
        for (; !(start == inited); init_words++) start();
        printf("{\"init\":{\"words\":%d,", init_words);
        p.dump();
        printf("},\"states\":[");
        const int gens = atoi(argv[7]);
        for (int g = 1; g <= gens; g++) {
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
    } else if (!strcmp(argv[1], "runs")) {
        const double box = atof(argv[5]);
        std::vector<double> lo(n, -box), up(n, box), guess(n, 0.);
        multivariate_problem prob { f, n, lo.data(), up.data() };
        const int seed0 = atoi(argv[6]), count = atoi(argv[7]);
        printf("[");
        for (int s = 0; s < count; s++) {
            Random::seed((unsigned) (seed0 + s));
            Probe p(atoi(argv[8]), atof(argv[9]), np);
            const auto sol = p.optimize(prob, guess.data());
            printf("%s{\"seed\":%d,\"fev\":%d,\"converged\":%d,\"fabest\":\"%a\"}", s ? "," : "", seed0 + s,
                    sol._fev, sol._converged ? 1 : 0, p.fabest());
        }
        printf("]\n");
    } else {
        std::vector<double> lo(n, -5.), up(n, 5.), guess(n, 0.);
        multivariate_problem prob { f, n, lo.data(), up.data() };
        Random::seed(1u);
        const int gens = atoi(argv[5]);
        Probe p(100 * np * (gens + 20), 0., np);
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
         os.path.join(src, "multivariate/pso/slpso.cpp"), os.path.join(src, "blas.cpp"), "-lm"])
    return exe


def box_of(rec):
    if rec["box"] == "percoord":
        from _boxes import percoord_box
        return [list(v) for v in percoord_box(rec["n"])]
    return [-rec["box"]] * rec["n"], [rec["box"]] * rec["n"]


def replay(rec):
    """the record through tests/slpso_model.py: (reproduced bit for bit, events, smallest gap, mfes ok)"""
    import numpy as np
    import chol_model
    import jaya_model as jm
    import slpso_model as sm

    def h(v):
        return np.array([float.fromhex(s) for s in v])

    n, np_ = rec["n"], rec["np"]
    lo, up = box_of(rec)
    m = sm.Slpso(chol_model.objective(rec["objective"], n), lo, up, np_, rec["mfev"],
                 rec["stol"], Ufmax=rec["Ufmax"])
    m.trace = True
    m.start(h(rec["init"]["x"]).reshape(np_, n), rec["init"]["perm"])
    have, saved, ok_mfes = False, 0., True
    for st in rec["states"]:
        w = jm.Words(st["words"])
        w.have, w.saved = have, saved
        m.iterate(sm.WordsSource(w, n, np_))
        have, saved = w.have, w.saved
        if not w.exhausted():
            return False, set(), 0., False
        got = m.state()
        for k in sm.Slpso.KEYS:
            want = st[k]
            if isinstance(want, list):
                want = h(want) if want and isinstance(want[0], str) else np.array(want, float)
                if np.asarray(got[k], float).tobytes() != want.tobytes():
                    return False, set(), 0., False
            elif isinstance(want, str):
                if float(got[k]).hex() != want:
                    return False, set(), 0., False
            elif int(got[k]) != want:
                return False, set(), 0., False
        r = m.mfes_real
        if abs(r - round(r)) < MIN_GAP and r != np_:
            ok_mfes = False
    rec["repairs"] = dict(m.repairs)
    return True, set(m.events), min(m.gaps) if m.gaps else 1., ok_mfes


def box_arg(box, n):
    """the harness's box argument: a number, or for "percoord" the bounds of tests/_boxes.py, "l0,..|u0,.." """
    if box != "percoord":
        return repr(box)
    from _boxes import percoord_box
    lo, up = percoord_box(n)
    return ",".join(repr(float(v)) for v in lo) + "|" + ",".join(repr(float(v)) for v in up)


def record(exe, name, n, np_, obj, box, ufmax, seed, generations=GENERATIONS, need_repairs=0):
    mfev = 40 * np_
    for attempt in range(64):
        out = subprocess.check_output(
            [exe, "steps", str(OBJ_IDS[obj]), str(n), str(np_), box_arg(box, n), str(seed + 1000 * attempt),
             str(generations), repr(ufmax), str(mfev), repr(STOL)])
        rec = _norm(json.loads(out))
        rec.update({"name": name, "n": n, "np": np_, "objective": obj, "box": box,
                    "Ufmax": ufmax, "mfev": mfev, "stol": STOL, "seed": seed + 1000 * attempt})
        same, events, gap, ok_mfes = replay(rec)
        if not same:
            sys.exit("%s: tests/slpso_model.py does not reproduce the reference (seed %d)" % (name, rec["seed"]))
        if gap >= MIN_GAP and ok_mfes and min(rec["repairs"].values()) >= need_repairs:
            break
    else:
        sys.exit("%s: no seed without a close decision" % name)
    rec["events"] = sorted(events)
    rec["min_gap"] = gap
    compact(rec)
    return rec


def compact(rec):
    """the record in the fixture's form.  The words of a generation are the outputs of std::mt19937 under
    the record's seed from where the generation before it stopped: the fixture keeps their number and
    their CRC-32 (as little-endian 32-bit words), after this function has checked that
    slpso_model.Mt19937Words makes exactly the recorded words from the seed.  The float arrays of a state
    keep the entries that changed (slpso_model.pack_states); floats that stand alone stay float.hex."""
    import slpso_model as sm
    live = sm.Mt19937Words(rec["seed"])
    live.take(rec["init"]["words"])
    for st in rec["states"]:
        words = st["words"]
        if live.take(len(words)) != words:
            sys.exit("%s: the seed does not give back the recorded words" % rec["name"])
        st["words"] = {"count": len(words), "crc32": sm.words_crc(words)}
    states = [rec["init"]] + rec["states"]
    for st in states:
        for k in sm.FLOAT_KEYS:
            st[k] = [float.fromhex(v) for v in st[k]]
    sm.pack_states(states)


def generate(ref="/root/reference"):
    tmp = tempfile.mkdtemp(prefix="slpso_golden_")
    try:
        exe = build(ref, tmp)
        steps = [record(exe, *shape) for shape in SHAPES]
        seen = set().union(*(set(r["events"]) for r in steps))
        if not WANTED <= seen:
            sys.exit("the steps runs never take: %s" % sorted(WANTED - seen))
        b = RUNS
        runs = dict(RUNS)
        for obj in ("sphere", "rosenbrock"):
            out = subprocess.check_output(
                [exe, "runs", str(OBJ_IDS[obj]), str(b["n"]), str(b["np"]), repr(b["box"]), str(b["seed0"]),
                 str(b["count"]), str(b["mfev"]), repr(b["stol"])])
            runs[obj] = _norm(json.loads(out))
        return {"steps": steps, "runs": runs, "signature": SIGNATURE}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def generate_percoord(ref="/root/reference"):
    """tests/golden/slpso_percoord.json: PERCOORD alone, with at least three coordinates redrawn at each wall ("repairs")"""
    tmp = tempfile.mkdtemp(prefix="slpso_golden_")
    try:
        rec = record(build(ref, tmp), *PERCOORD, generations=PERCOORD_GENERATIONS, need_repairs=3)
        return {"steps": [rec]}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def time_reference(ref="/root/reference"):
    """ms per generation of the reference on one core: the shape of scripts/bench_slpso.py"""
    tmp = tempfile.mkdtemp(prefix="slpso_time_")
    try:
        exe = build(ref, tmp)
        for n, np_, gens in ((128, 20, 2000),):
            runs = [json.loads(subprocess.check_output(
                [exe, "time", str(OBJ_IDS["rosenbrock"]), str(n), str(np_), str(gens)])) for _ in range(5)]
            ms = sorted(r["ms_per_generation"] for r in runs)
            print("n = %d, np = %d: %.4f ms per generation (median of 5 runs of %d; min %.4f, max %.4f), "
                  "%.1f evaluations per generation" % (n, np_, ms[2], gens, ms[0], ms[-1],
                                                       runs[0]["evals_per_generation"]))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def dumps(data):
    return json.dumps(data, sort_keys=True, separators=(",", ":")) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "slpso_runs.json"))
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--percoord", action="store_true",
                    help="write the per-coordinate record alone, to tests/golden/slpso_percoord.json")
    a = ap.parse_args()
    if not os.path.isdir(os.path.join(a.ref, "src")):
        sys.exit("the reference sources are not at %s" % a.ref)
    if a.time:
        time_reference(a.ref)
        return
    if a.percoord and a.out.endswith("slpso_runs.json"):
        a.out = os.path.join(ROOT, "tests", "golden", "slpso_percoord.json")
    data = generate_percoord(a.ref) if a.percoord else generate(a.ref)
    text = dumps(data)
    with open(a.out, "w") as fh:
        fh.write(text)
    for rec in data["steps"]:
        print("%s: seed %d, smallest gap %.2e, %s" % (rec["name"], rec["seed"], rec["min_gap"], " ".join(rec["events"])))
    print("wrote %s (%d bytes)" % (a.out, len(text)))


if __name__ == "__main__":
    main()
