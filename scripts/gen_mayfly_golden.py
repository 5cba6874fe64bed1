#!/usr/bin/env python3
"""Records runs of the REAL MayflySearch of the reference into tests/golden/mayfly_runs.json (needs the
reference's sources and g++; run on the development machine, never where the GPU tests run).

    python scripts/gen_mayfly_golden.py [--ref /root/reference] [--out tests/golden/mayfly_runs.json]
    python scripts/gen_mayfly_golden.py --time     # the reference's ms per generation on one core

A small harness (the C++ text below, this project's own) is compiled in a temporary directory against the
reference's mayfly.cpp with the flags of oracle/Makefile (-O2 -ffp-contract=off).  It seeds
effolkronium::random_static::seed(k) and drives a subclass probe (the members of MayflySearch are protected).

Per shape the harness prints the swarms after init() and, for each of the first generations, the raw 32-bit
words the generation took from the global mt19937 (counted on a copy of the engine), every point handed to
the objective in order with its value, and the whole state after the generation.  Every recorded run is
replayed here through tests/mayfly_model.py over the recorded words and must match bit for bit: every point,
every value, every field of every fly, best, fbest and the schedule.

What the fixture keeps ("steps") is what a test needs to do the same without the reference, compactly: the
words are the outputs of std::mt19937 seeded with the shape's seed, which tests/mayfly_model.mt19937_words
regenerates (checked here word for word), so only their COUNT per generation is stored; of a generation fbest, the evaluation that took it last, and
CRC-32 sums of the points handed to the objective, of their values and of the state after it (the packed
doubles), which pin every bit of all three.  A state of the largest shape is 21 450 doubles and a generation's words up to 17 000: stored
verbatim, 16 generations of it would be several MiB.

The reference builds its flies as mayfly { v, x, bx, f, f } over a struct declared _x, _v, _bx, so every fly
starts at the ORIGIN with the drawn point as its velocity: the swarms cluster from the first generation on,
an offspring of two parents at one point is that point with v = 0, and values that tie between records that
differ are common.  Beyond 16 records std::sort is not stable, so the model walks libstdc++'s introsort
(mayfly_model.std_sort) to follow the reference through such ties, and a generation is marked "ok" -- one
the device can be held to -- when no sort of it meets two records at different positions within 1e-6 relative
in f (exact duplicates are the rule and harmless), and "stable" when, besides, every sort of it is the
stable order's (the swarms' sorts up to records equal in every field, the selections' rank for rank): then
the state after the selection is the device's too; otherwise the device's selection is held to the model's
stable order from the reference's state before it.  A shape's seed moves on until 12 of its 20 generations
are ok, or the seed with the most is kept (at least 4: the swarms collapse onto each other within a few
generations at n >= 33, and close values are then the rule).  The paths the model met in the ok generations
are counted and stored ("paths"); each must be met at least twice over the shapes.
"bands": the sorted final f(best) of 256 seeds (1000 + s) at a fixed budget on the sphere and on Rosenbrock,
n = 10, np = 20.  Before they are stored, the two disjoint halves of the reference's own runs must pass the
comparison the device has to pass (the median of log10 f of one half inside the quartiles of the other).
"signature": the argument names and defaults of the binding the reference writes out, commented away, at
py/multivariate_py.cpp:236-246.  Floats are float.hex strings.  The fixture holds numbers and names only.
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

# (name, n, np, objective, box, seed, generations, parameters that differ from the defaults; "lower": the
# lower bound where it is not -box)
SHAPES = [
    ("n1_np2", 1, 2, "sphere", 4., 11, 20, {}),
    ("n2_np4", 2, 4, "rosenbrock", 3., 22, 20, {}),
    ("n3_np6", 3, 6, "schwefel12", 5., 33, 20, {"lower": -0.25}),     # (the origin next to the lower bound)
    ("n17_np10", 17, 10, "rosenbrock", 5., 44, 20, {}),
    ("n17_np10_mut", 17, 10, "schwefel12", 5., 55, 20, {"pmutnp": 0.3}),
    ("n33_np40_pgb", 33, 40, "rosenbrock", 5., 66, 20, {"pgb": True}),
    ("n65_np66", 65, 66, "rosenbrock", 5., 77, 20, {"pmutdim": 0.1}),
]
# one short record under the per-coordinate box of tests/_boxes.py (the harness is handed its bounds, box_arg): vmax, the
# mutation's sigma and the clamps with bounds that differ in every coordinate
PERCOORD = ("percoord_n11_np6", 11, 6, "sphere", "percoord", 88, 5, {"pmutnp": 0.3})
MFEV = 1000000
SEEDS_TRIED = 40
MIN_OK, GOOD_OK = 4, 12     # of a shape's recorded generations, those the device can be held to: at least, enough
PATHS = ("f_attract", "f_random", "m_attract", "m_dance", "improve_not_last", "short_window", "aliased",
         "clamp_box", "clamp_vmax")
OBJ_IDS = {"sphere": 0, "rosenbrock": 1, "rastrigin": 2, "ellipsoid": 3, "ackley": 4,
           "griewank": 5, "cigar": 6, "discus": 7, "diffpow": 8, "schwefel12": 9}
BANDS = dict(n=10, np=20, mfev=6000, box=5., seed0=1000, count=256)
STATE_KEYS = ("males_x", "males_v", "males_bx", "males_f", "males_bf", "females_x", "females_v", "females_f",
              "xbest", "fbest", "g", "dance", "fl")     # (mayfly_model.STATE_KEYS: what state_crc sums)

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
#include "multivariate/mayfly/mayfly.h"

using Random = effolkronium::random_static;

static void vec(const char *k, const std::vector<double> &v, bool last = false)
{
    printf("\"%s\":[", k);
    for (size_t i = 0; i < v.size(); i++) printf("%s\"%a\"", i ? "," : "", v[i]);
    printf("]%s", last ? "" : ",");
}

struct Probe: public MayflySearch {
    using MayflySearch::MayflySearch;
    void dump()
    {
        std::vector<double> mx, mv, mbx, mf, mbf, fx, fv, ff;
        for (auto &p : _males) {
            mx.insert(mx.end(), p->_x.begin(), p->_x.end());
            mv.insert(mv.end(), p->_v.begin(), p->_v.end());
            mbx.insert(mbx.end(), p->_bx.begin(), p->_bx.end());
            mf.push_back(p->_f);
            mbf.push_back(p->_bf);
        }
        for (auto &p : _females) {
            fx.insert(fx.end(), p->_x.begin(), p->_x.end());
            fv.insert(fv.end(), p->_v.begin(), p->_v.end());
            ff.push_back(p->_f);
        }
        vec("males_x", mx); vec("males_v", mv); vec("males_bx", mbx); vec("males_f", mf); vec("males_bf", mbf);
        vec("females_x", fx); vec("females_v", fv); vec("females_f", ff); vec("xbest", _best);
        vec("fbest", { _fbest }); vec("g", { _g }); vec("dance", { _dance }); vec("fl", { _fl });
        printf("\"fev\":%d,\"it\":%d,\"itmax\":%d,\"nmut\":%d", _fev, _it, _itmax, _nmut);
    }
    double fbest() const { return _fbest; }
    int fev() const { return _fev; }
};

struct Ctx { int obj, n; std::vector<double> aux; std::vector<double> log; bool keep; };

static void words_between(std::mt19937 before, const std::mt19937 &after)
{
    printf("\"words\":[");
    for (int i = 0; !(before == after); i++) printf("%s%u", i ? "," : "", (unsigned) before());
    printf("],");
}

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
    // steps <obj> <n> <np> <box> <seed> <generations> <mfev> <pmutnp> <pmutdim> <pgb> <lower>
    // bands <obj> <n> <np> <mfev> <box> <seed0> <count>
    // time  <obj> <n> <np> <generations>
    Ctx c { atoi(argv[2]), atoi(argv[3]), {}, {}, false };
    const int n = c.n, np = atoi(argv[4]);
    c.aux.resize(n);
    bbo_objective_aux(c.obj, n, c.aux.data());
    multivariate f = [&c](const double *x) {
        const double v = bbo_objective_eval(c.obj, c.n, x, c.aux.data());
        if (c.keep) {
            c.log.insert(c.log.end(), x, x + c.n);
            c.log.push_back(v);
        }
        return v;
    };
    if (!strcmp(argv[1], "steps")) {
        const double box = atof(argv[5]);
        std::vector<double> lo(n, atof(argv[12])), up(n, box), guess(n, 0.);
        bounds_arg(argv[5], lo, up);
        multivariate_problem prob { f, n, lo.data(), up.data() };
        Random::seed((unsigned) atoi(argv[6]));
        Probe p(np, atoi(argv[8]), 1., 1.5, 1.5, 2., 5., 0.8, 1., 0.99, 0.8, 0.8, 0.1, 0.1, atof(argv[10]),
                atof(argv[9]), 0.95, atoi(argv[11]) != 0);
        c.keep = true;
        auto before = Random::get_engine();
        p.init(prob, guess.data());
        printf("{\"init\":{");
        words_between(before, Random::get_engine());
        vec("evals", c.log);
        p.dump();
        printf("},\"states\":[");
        const int gens = atoi(argv[7]);
        for (int g = 1; g <= gens; g++) {
            before = Random::get_engine();
            c.log.clear();
            p.iterate();
            printf("%s{", g > 1 ? "," : "");
            words_between(before, Random::get_engine());
            vec("evals", c.log);
            p.dump();
            printf("}");
        }
        printf("]}\n");
    } else if (!strcmp(argv[1], "bands")) {
        const double box = atof(argv[6]);
        std::vector<double> lo(n, -box), up(n, box), guess(n, 0.);
        multivariate_problem prob { f, n, lo.data(), up.data() };
        const int seed0 = atoi(argv[7]), count = atoi(argv[8]);
        std::vector<double> out;
        printf("{\"fev\":[");
        for (int s = 0; s < count; s++) {
            Random::seed((unsigned) (seed0 + s));
            Probe p(np, atoi(argv[5]));
            p.optimize(prob, guess.data());
            out.push_back(p.fbest());
            printf("%s%d", s ? "," : "", p.fev());
        }
        printf("],");
        vec("fbest", out, true);
        printf("}\n");
    } else {
        std::vector<double> lo(n, -5.), up(n, 5.), guess(n, 0.);
        multivariate_problem prob { f, n, lo.data(), up.data() };
        Random::seed(1u);
        const int gens = atoi(argv[5]);
        Probe p(np, 1 << 30);
        p.init(prob, guess.data());
        for (int g = 0; g < 10; g++) p.iterate();
        const int fev0 = p.fev();
        const auto t0 = std::chrono::steady_clock::now();
        for (int g = 0; g < gens; g++) p.iterate();
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        printf("{\"ms_per_generation\":%.6f,\"evaluations_per_generation\":%.2f}\n", ms / gens,
                (double) (p.fev() - fev0) / gens);
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
         os.path.join(src, "multivariate/mayfly/mayfly.cpp"), "-lm"])
    return exe


def _hx(v):
    return [float.fromhex(s) for s in v]


def crc(values):
    import mayfly_model as mm
    return mm.crc(values)


def state_crc(state):
    import mayfly_model as mm
    return mm.state_crc(state)


def params_of(shape):
    import mayfly_model as mm
    par = dict(mm.DEFAULTS)
    par.update(shape[7])
    par.pop("lower", None)
    return par


def lower_of(shape):
    if shape[4] == "percoord":
        return "percoord"
    return shape[7].get("lower", -shape[4])


def bounds_of(shape):
    n, box = shape[1], shape[4]
    if box == "percoord":
        from _boxes import percoord_box
        return [list(v) for v in percoord_box(n)]
    return [lower_of(shape)] * n, [box] * n


def box_arg(box, n):
    """the harness's box argument: a number, or for "percoord" the bounds of tests/_boxes.py, "l0,..|u0,.." """
    if box != "percoord":
        return repr(box)
    from _boxes import percoord_box
    lo, up = percoord_box(n)
    return ",".join(repr(float(v)) for v in lo) + "|" + ",".join(repr(float(v)) for v in up)


def run_shape(exe, shape, seed):
    name, n, np_, obj, box, _, gens, _ = shape
    par = params_of(shape)
    out = subprocess.check_output(
        [exe, "steps", str(OBJ_IDS[obj]), str(n), str(np_), box_arg(box, n), str(seed), str(gens), str(MFEV),
         repr(par["pmutnp"]), repr(par["pmutdim"]), str(int(par["pgb"])), repr(lower_of(shape))])
    return _norm(json.loads(out))


def replay(rec, shape, seed):
    """the recorded run through tests/mayfly_model.py over its words, bit for bit; returns the fixture's
    record, or None when a sort met two close records that differ"""
    import chol_model
    import jaya_model
    import mayfly_model as mm
    name, n, np_, obj, box, _, gens, _ = shape
    par = params_of(shape)
    counts = [len(rec["init"]["words"])] + [len(st["words"]) for st in rec["states"]]
    words = list(rec["init"]["words"])
    for st in rec["states"]:
        words += st["words"]
    assert mm.mt19937_words(seed, len(words)) == words, "std::mt19937(seed) is not what numpy regenerates"
    w = jaya_model.Words(words)
    lo, up = bounds_of(shape)
    m = mm.Mayfly(chol_model.objective(obj, n), n, np_, lo, up, MFEV, **par)
    src = mm.WordsSource(w, n)

    def same(st, tag):
        ev = _hx(st["evals"])
        assert [v for x, fx in m.evals for v in x + [fx]] == ev, tag + "evals"
        got = m.state()
        for k in STATE_KEYS:
            a = [v for r in got[k] for v in (r if isinstance(r, list) else [r])]
            assert a == _hx(st[k]), tag + k
        assert (m.fev, m.it, m.itmax, m.nmut) == (st["fev"], st["it"], st["itmax"], st["nmut"]), tag

    m.init_words(w)
    assert w.i == counts[0]
    same(rec["init"], name + " init ")
    out = {"name": name, "n": n, "np": np_, "objective": obj, "box": box,
           "lower": lower_of(shape), "mfev": MFEV,
           "seed": seed, "params": {k: v for k, v in shape[7].items() if k != "lower"}, "nwords": counts, "nmut": m.nmut,
           "init": {"values_crc": crc(fx for _, fx in m.evals), "points_crc": crc(v for x, _ in m.evals for v in x),
                    "state_crc": state_crc(m.state()), "fbest": m.fbest.hex()},
           "states": []}
    at = counts[0]
    paths = {k: 0 for k in PATHS}
    for g, st in enumerate(rec["states"]):
        before = (m.close_distinct, m.unstable, dict(m.paths))
        m.iterate(src)
        at += counts[g + 1]
        assert w.i == at, "%s generation %d: the model read %d words, the reference %d" % (name, g, w.i, at)
        same(st, "%s generation %d " % (name, g))
        # "ok": a generation the device can be held to -- no two records at different positions within 1e-6
        # relative in any sort; "stable": every sort of it as the stable order sorts it, so that the state
        # after the selection is the device's too, and the chain landed what the in-place loop landed
        ok = m.close_distinct == before[0]
        stable = m.unstable == before[1]
        assert m.chain_ok or not (ok and stable), "%s generation %d: the chain is not the in-place loop" % (name, g)
        if ok:
            for k in PATHS:
                paths[k] += m.paths[k] - before[2][k]
        out["states"].append({"values_crc": crc(fx for _, fx in m.evals),
                              "points_crc": crc(v for x, _ in m.evals for v in x),
                              "state_crc": state_crc(m.state()), "fbest": m.fbest.hex(), "took": m.took,
                              "fev": m.fev, "dup_m": m.duplicates(True), "dup_f": m.duplicates(False),
                              "ok": bool(ok), "stable": bool(ok and stable)})
    out["paths"] = paths
    return out


def record(exe, shape, need=(), good_ok=GOOD_OK):
    """the first seed with at least MIN_OK generations the device can be held to (and every path of `need`)"""
    name, seed0 = shape[0], shape[5]
    best = None
    for attempt in range(SEEDS_TRIED):
        seed = seed0 + 1000 * attempt
        out = replay(run_shape(exe, shape, seed), shape, seed)
        good = sum(st["ok"] for st in out["states"])
        if any(out["paths"][k] < 1 for k in need):
            continue
        if best is None or good > best[0]:
            best = (good, out)
        if good >= good_ok:
            break
    if best is None or best[0] < MIN_OK:
        sys.exit("%s: no seed with %d comparable generations" % (name, MIN_OK))
    return best[1]


def generate_percoord(ref="/root/reference"):
    """tests/golden/mayfly_percoord.json: PERCOORD alone, with both clamps in it"""
    tmp = tempfile.mkdtemp(prefix="mayfly_golden_")
    try:
        return {"steps": [record(build(ref, tmp), PERCOORD, need=("clamp_box", "clamp_vmax"), good_ok=PERCOORD[6])]}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def signature(ref):
    """the argument names and defaults of the commented binding (py/multivariate_py.cpp:236-246)"""
    with open(os.path.join(ref, "py", "multivariate_py.cpp")) as fh:
        text = fh.read()
    body = text[text.index("build_mayfly"):]
    body = body[:body.index("//}")].replace("//", " ")
    sig = []
    for name, default in re.findall(r'"(\w+)"_a\s*(?:=\s*([\w.+-]+))?', " ".join(body.split())):
        if not default:
            sig.append({"name": name, "required": True})
        elif default in ("true", "false"):
            sig.append({"name": name, "required": False, "default": default == "true"})
        else:
            sig.append({"name": name, "required": False, "default": float(default)})
    return sig


def halves_pass(ref_f):
    """the band comparison of the GPU test (tests/test_hees_model.band) between the two disjoint halves of
    the reference's own runs, both ways"""
    import numpy as np
    a, b = np.log10(np.asarray(ref_f[0::2]) + 1e-300), np.log10(np.asarray(ref_f[1::2]) + 1e-300)
    for dev, ref in ((a, b), (b, a)):
        q1, q3 = np.percentile(ref, [25, 75])
        if not q1 <= np.median(dev) <= q3:
            return False
    return True


def generate(ref="/root/reference"):
    tmp = tempfile.mkdtemp(prefix="mayfly_golden_")
    try:
        exe = build(ref, tmp)
        steps, have = [], {k: 0 for k in PATHS}
        for shape in SHAPES:
            rec = record(exe, shape)
            for k in PATHS:
                have[k] += rec["paths"][k]
            steps.append(rec)
        for k in PATHS:
            if have[k] < 2:
                sys.exit("path %s met %d times only" % (k, have[k]))
        bands = dict(BANDS)
        b = BANDS
        for obj in ("sphere", "rosenbrock"):
            o = json.loads(subprocess.check_output(
                [exe, "bands", str(OBJ_IDS[obj]), str(b["n"]), str(b["np"]), str(b["mfev"]), repr(b["box"]),
                 str(b["seed0"]), str(b["count"])]))
            fb = _hx(o["fbest"])
            if not halves_pass(fb):
                sys.exit("bands: the halves of the reference's own %s runs do not pass the comparison" % obj)
            bands[obj] = [v.hex() for v in sorted(fb)]
            bands[obj + "_fev"] = [min(o["fev"]), max(o["fev"])]
        return {"steps": steps, "bands": bands, "signature": signature(ref), "paths": have}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def time_reference(ref="/root/reference"):
    """ms per generation of the reference on one core: the shapes of scripts/bench_mayfly.py"""
    tmp = tempfile.mkdtemp(prefix="mayfly_time_")
    try:
        exe = build(ref, tmp)
        for n, np_, gens in ((128, 20, 2000), (128, 256, 200)):
            runs = [json.loads(subprocess.check_output(
                [exe, "time", str(OBJ_IDS["rosenbrock"]), str(n), str(np_), str(gens)])) for _ in range(5)]
            best = min(runs, key=lambda r: r["ms_per_generation"])
            print("n = %d, np = %d: %.4f ms per generation, %.1f evaluations per generation (best of 5 runs of %d)"
                  % (n, np_, best["ms_per_generation"], best["evaluations_per_generation"], gens))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def dumps(data):
    return json.dumps(data, sort_keys=True, separators=(",", ":")) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "mayfly_runs.json"))
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--percoord", action="store_true",
                    help="write the per-coordinate record alone, to tests/golden/mayfly_percoord.json")
    a = ap.parse_args()
    if not os.path.isdir(os.path.join(a.ref, "src")):
        sys.exit("the reference sources are not at %s" % a.ref)
    if a.time:
        time_reference(a.ref)
        return
    if a.percoord and a.out.endswith("mayfly_runs.json"):
        a.out = os.path.join(ROOT, "tests", "golden", "mayfly_percoord.json")
    data = generate_percoord(a.ref) if a.percoord else generate(a.ref)
    text = dumps(data)
    with open(a.out, "w") as fh:
        fh.write(text)
    for rec in data["steps"]:
        print("%s: seed %d, paths %s" % (rec["name"], rec["seed"], rec["paths"]))
    if "paths" in data:
        print("paths over all shapes: %s" % data["paths"])
    print("wrote %s (%d bytes)" % (a.out, len(text)))


if __name__ == "__main__":
    main()
