#!/usr/bin/env python3
"""Records runs of the REAL PikaiaSearch of the reference into tests/golden/pikaia_runs.json (needs the
reference's sources and g++; run on the development machine, never where the GPU tests run).

    python scripts/gen_pikaia_golden.py [--ref /root/reference] [--out tests/golden/pikaia_runs.json]
    python scripts/gen_pikaia_golden.py --time     # the reference's ms per generation on one core

A small harness (the C++ text below, this project's own) is compiled in a temporary directory against the
reference's pikaia.cpp with the flags of oracle/Makefile (-O2 -ffp-contract=off).  It seeds
effolkronium::random_static::seed(k) and drives a subclass probe (the members of PikaiaSearch are protected).
The objective f is wrapped as the device's default mode wraps it: u -> -f(lower + u (upper - lower)), one
multiply and one add per coordinate.

Per shape the harness prints, after init() and after each generation, how many 32-bit words the global mt19937
gave (counted on a copy of the engine), every point handed to the objective in order with its value, and the
state (_oldph, _fitns, _ifit, _pmut, _fev, _ig).  Every recorded run is replayed here through
tests/pikaia_model.py (order="rqsort") over the words of std::mt19937(seed), which
tests/mayfly_model.mt19937_words regenerates, and must match bit for bit.

What the fixture keeps per generation: the word count, pmut, the elite decision, fev, and CRC-32 sums of the new
phenotypes, of the values and of the state after it (phenotypes, fitness, pmut) and of the rank order, which pin
every bit.  A generation is "ok" -- one the device can be held to -- when no two rows that differ have values
within 1e-6 relative, the elite comparison is not within 1e-6 relative and rdif is not within 1e-9 of a
threshold.  A shape's seed moves on (by 1000, at most 40 times) until 12 of its 20 generations are ok.  The
paths the model met are counted ("paths"); each must be met at least twice over the shapes.
"bands": the sorted final best f of 256 seeds (1000 + s) for two settings on the sphere and on Rosenbrock; before
they are stored the two halves of the reference's own runs must pass tests/test_hees_model.band against each
other; they are kept to seven digits, which is all a comparison of quartiles reads.  "signature": the argument names and defaults of the constructor in pikaia.h.  "pow10": std::pow(10., nd)
and std::pow(10., -nd) per nd.  Floats are float.hex strings.  The fixture holds numbers and names only.
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

# (name, n, np, nd, imut, ielite, objective, seed, parameters that differ from the defaults)
SHAPES = [
    ("n1_np8", 1, 8, 4, 1, 0, "sphere", 11, {}),
    ("n2_np10", 2, 10, 6, 2, 1, "rosenbrock", 22, {}),
    ("n3_np20", 3, 20, 5, 5, 0, "rosenbrock", 33, {}),
    ("n17_np32", 17, 32, 6, 3, 1, "rosenbrock", 44, {}),
    ("n33_np64_creep", 33, 64, 9, 4, 0, "rosenbrock", 55, {}),
    ("n65_np66", 65, 66, 6, 6, 1, "rosenbrock", 66, {}),
    ("n2_np12_fdif", 2, 12, 3, 3, 1, "rosenbrock", 77, {"fdif": 0.5}),
    ("n4_np16_dense", 4, 16, 4, 4, 0, "rosenbrock", 88, {"pcross": 1., "pmut": 0.05}),
]
LOWER, UPPER, GENS = -3.25, 5., 20
SEEDS_TRIED, GOOD_OK = 40, 12
OBJ_IDS = {"sphere": 0, "rosenbrock": 1}
BANDS = dict(n=10, np=50, nd=6, ngen=60, lower=LOWER, upper=UPPER, seed0=1000, count=256,
             settings=[dict(imut=2, ielite=0), dict(imut=6, ielite=1)])

HARNESS = r"""
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "objectives.h"
#include "random.hpp"
#include "multivariate/multivariate.h"
#include "multivariate/pikaia/pikaia.h"

using Random = effolkronium::random_static;

static void vec(const char *k, const std::vector<double> &v)
{
    printf("\"%s\":[", k);
    for (size_t i = 0; i < v.size(); i++) printf("%s\"%a\"", i ? "," : "", v[i]);
    printf("],");
}

struct Probe: public PikaiaSearch {
    using PikaiaSearch::PikaiaSearch;
    void dump()
    {
        vec("ph", _oldph);
        vec("fitns", _fitns);
        printf("\"ifit\":[");
        for (int i = 0; i < _np; i++) printf("%s%d", i ? "," : "", _ifit[i] - 1);
        printf("],\"pmut\":\"%a\",\"fev\":%d,\"ig\":%d", _pmut, _fev, _ig);
    }
    double best() const { return _fitns[_ifit[_np - 1] - 1]; }
    int fev() const { return _fev; }
};

struct Ctx { int obj, n; double lo, up; std::vector<double> aux, x, log; bool keep; };

static long words_between(std::mt19937 before, const std::mt19937 &after)
{
    long k = 0;
    for (; !(before == after); k++) before();
    return k;
}

int main(int argc, char **argv)
{
    // steps <obj> <n> <np> <nd> <imut> <ielite> <seed> <gens> <lower> <upper> <pcross> <pmut> <fdif>
    // bands <obj> <n> <np> <nd> <imut> <ielite> <seed0> <count> <lower> <upper> <ngen>
    // time  <obj> <n> <np> <nd> <gens>
    Ctx c { atoi(argv[2]), atoi(argv[3]), 0., 1., {}, {}, {}, false };
    const int n = c.n, np = atoi(argv[4]), nd = atoi(argv[5]);
    c.aux.resize(n);
    c.x.resize(n);
    bbo_objective_aux(c.obj, n, c.aux.data());
    multivariate f = [&c](const double *u) {
        for (int i = 0; i < c.n; i++) {
            const double w = c.up - c.lo;
            const double s = u[i] * w;
            c.x[i] = c.lo + s;
        }
        const double v = bbo_objective_eval(c.obj, c.n, c.x.data(), c.aux.data());
        if (c.keep) {
            c.log.insert(c.log.end(), c.x.begin(), c.x.end());
            c.log.push_back(v);
        }
        return -v;
    };
    std::vector<double> lo(n, 0.), up(n, 1.), guess(n, 0.);
    multivariate_problem prob { f, n, lo.data(), up.data() };
    if (!strcmp(argv[1], "steps")) {
        c.lo = atof(argv[10]);
        c.up = atof(argv[11]);
        Random::seed((unsigned) atoi(argv[8]));
        Probe p(np, 1 << 20, nd, atof(argv[12]), atoi(argv[6]), atof(argv[13]), 0.0005, 0.25, atof(argv[14]), 1,
                atoi(argv[7]));
        c.keep = true;
        auto before = Random::get_engine();
        p.init(prob, guess.data());
        printf("{\"init\":{\"nwords\":%ld,", words_between(before, Random::get_engine()));
        vec("evals", c.log);
        p.dump();
        printf("},\"states\":[");
        const int gens = atoi(argv[9]);
        for (int g = 1; g <= gens; g++) {
            before = Random::get_engine();
            c.log.clear();
            p.iterate();
            printf("%s{\"nwords\":%ld,", g > 1 ? "," : "", words_between(before, Random::get_engine()));
            vec("evals", c.log);
            p.dump();
            printf("}");
        }
        printf("]}\n");
    } else if (!strcmp(argv[1], "bands")) {
        c.lo = atof(argv[10]);
        c.up = atof(argv[11]);
        const int seed0 = atoi(argv[8]), count = atoi(argv[9]);
        std::vector<double> out;
        printf("{\"fev\":[");
        for (int s = 0; s < count; s++) {
            Random::seed((unsigned) (seed0 + s));
            Probe p(np, atoi(argv[12]), nd, 0.85, atoi(argv[6]), 0.005, 0.0005, 0.25, 1., 1, atoi(argv[7]));
            p.optimize(prob, guess.data());
            out.push_back(-p.best());
            printf("%s%d", s ? "," : "", p.fev());
        }
        printf("],");
        vec("fbest", out);
        printf("\"count\":%d}\n", count);
    } else {
        c.lo = -5.;
        c.up = 5.;
        Random::seed(1u);
        const int gens = atoi(argv[6]);
        Probe p(np, 1 << 20, nd);
        p.init(prob, guess.data());
        for (int g = 0; g < 3; g++) p.iterate();
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
         os.path.join(src, "multivariate/pikaia/pikaia.cpp"), "-lm"])
    return exe


def params_of(shape):
    import pikaia_model as pm
    par = dict(pm.DEFAULTS)
    par.update(shape[8])
    par["imut"], par["ielite"] = shape[4], shape[5]
    return par


def run_shape(exe, shape, seed):
    name, n, np_, nd, imut, ielite, obj, _, _ = shape
    par = params_of(shape)
    out = subprocess.check_output(
        [exe, "steps", str(OBJ_IDS[obj]), str(n), str(np_), str(nd), str(imut), str(ielite), str(seed), str(GENS),
         repr(LOWER), repr(UPPER), repr(par["pcross"]), repr(par["pmut"]), repr(par["fdif"])])
    return json.loads(out)


def replay(rec, shape, seed):
    """the recorded run through tests/pikaia_model.py over the words of std::mt19937(seed), bit for bit;
    returns the fixture's record"""
    import chol_model
    import jaya_model
    import mayfly_model
    import pikaia_model as pm
    name, n, np_, nd, imut, ielite, obj, _, _ = shape
    par = params_of(shape)
    counts = [rec["init"]["nwords"]] + [st["nwords"] for st in rec["states"]]
    w = jaya_model.Words(mayfly_model.mt19937_words(seed, sum(counts)))
    m = pm.Pikaia(chol_model.objective(obj, n), n, np_, 1 << 20, nd, [LOWER] * n, [UPPER] * n, **par)
    src = pm.WordsSource(w)

    def same(st, tag):
        assert [v for x, fx in m.evals for v in x + [fx]] == _hx(st["evals"]), tag + "evals"
        assert [v for r in m.ph for v in r] == _hx(st["ph"]), tag + "ph"
        assert m.fitns == _hx(st["fitns"]), tag + "fitns"
        assert m.order == st["ifit"], tag + "ifit"
        assert (m.pmut, m.fev, m.ig) == (float.fromhex(st["pmut"]), st["fev"], st["ig"]), tag + "scalars"

    m.init_words(w)
    assert w.i == counts[0], name + " init words"
    same(rec["init"], name + " init ")
    out = {"name": name, "n": n, "np": np_, "nd": nd, "imut": imut, "ielite": ielite, "objective": obj,
           "lower": LOWER, "upper": UPPER, "seed": seed, "params": dict(shape[8]), "nwords": counts,
           "init": {"values_crc": pm.crc(fx for _, fx in m.evals), "state_crc": m.state_crc(),
                    "order_crc": pm.crc(m.order)},
           "states": []}
    at = counts[0]
    for g, st in enumerate(rec["states"]):
        m.iterate(src)
        at += counts[g + 1]
        assert w.i == at, "%s generation %d: the model read %d words, the reference %d" % (name, g, w.i, at)
        same(st, "%s generation %d " % (name, g))
        out["states"].append({"newph_crc": pm.crc(v for r in m.ph for v in r),
                              "values_crc": pm.crc(fx for _, fx in m.evals), "state_crc": m.state_crc(),
                              "order_crc": pm.crc(m.order), "pmut": m.pmut.hex(), "elite": m.elite, "fev": m.fev,
                              "ok": bool(m.ok())})
    out["paths"] = dict(m.paths)
    return out


def record(exe, shape):
    """the first seed with at least GOOD_OK generations the device can be held to"""
    name, seed0 = shape[0], shape[7]
    for attempt in range(SEEDS_TRIED):
        seed = seed0 + 1000 * attempt
        out = replay(run_shape(exe, shape, seed), shape, seed)
        if sum(st["ok"] for st in out["states"]) >= GOOD_OK:
            return out
    sys.exit("%s: no seed of %d with %d comparable generations" % (name, SEEDS_TRIED, GOOD_OK))


def signature(ref):
    """the argument names and defaults of the constructor (pikaia.h:25-27)"""
    with open(os.path.join(ref, "src", "multivariate", "pikaia", "pikaia.h")) as fh:
        text = " ".join(fh.read().split())
    body = re.search(r"PikaiaSearch\(([^)]*)\);", text).group(1)
    sig = []
    for arg in body.split(","):
        mt = re.match(r"\s*(int|double)\s+(\w+)\s*(?:=\s*([\w.+-]+))?\s*$", arg)
        kind, name, default = mt.groups()
        if default is None:
            sig.append({"name": name, "required": True})
        else:
            sig.append({"name": name, "required": False, "default": float(default) if kind == "double" else int(default)})
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
    import math
    import pikaia_model as pm
    tmp = tempfile.mkdtemp(prefix="pikaia_golden_")
    try:
        exe = build(ref, tmp)
        steps, have = [], {k: 0 for k in pm.PATHS}
        for shape in SHAPES:
            rec = record(exe, shape)
            for k in pm.PATHS:
                have[k] += rec["paths"][k]
            steps.append(rec)
        for k in pm.PATHS:
            if have[k] < 2:
                sys.exit("path %s met %d times only (all: %s)" % (k, have[k], have))
        b = BANDS
        bands = dict(b)
        bands["runs"] = []
        for s in b["settings"]:
            for obj in ("sphere", "rosenbrock"):
                o = json.loads(subprocess.check_output(
                    [exe, "bands", str(OBJ_IDS[obj]), str(b["n"]), str(b["np"]), str(b["nd"]), str(s["imut"]),
                     str(s["ielite"]), str(b["seed0"]), str(b["count"]), repr(b["lower"]), repr(b["upper"]),
                     str(b["ngen"])]))
                fb = _hx(o["fbest"])
                if not halves_pass(fb):
                    sys.exit("bands: the halves of the reference's own %s runs do not pass the comparison" % obj)
                assert set(o["fev"]) == {b["np"] + b["ngen"] * (b["np"] + 1)}
                bands["runs"].append(dict(s, objective=obj, fbest=[float("%.7g" % v) for v in sorted(fb)], fev=o["fev"][0]))
        pow10 = {str(nd): [math.pow(10., nd).hex(), math.pow(10., -nd).hex()] for nd in range(1, 10)}
        return {"steps": steps, "bands": bands, "signature": signature(ref), "paths": have, "pow10": pow10}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def time_reference(ref="/root/reference"):
    """ms per generation of the reference on one core: the shapes of scripts/bench_pikaia.py"""
    tmp = tempfile.mkdtemp(prefix="pikaia_time_")
    try:
        exe = build(ref, tmp)
        for n, np_, gens in ((128, 256, 100), (128, 4096, 10)):
            runs = [json.loads(subprocess.check_output(
                [exe, "time", str(OBJ_IDS["rosenbrock"]), str(n), str(np_), "6", str(gens)])) for _ in range(5)]
            best = min(runs, key=lambda r: r["ms_per_generation"])
            print("n = %d, np = %d, nd = 6: %.4f ms per generation, %.1f evaluations per generation (best of 5 runs of %d)"
                  % (n, np_, best["ms_per_generation"], best["evaluations_per_generation"], gens))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def dumps(data):
    return json.dumps(data, sort_keys=True, separators=(",", ":")) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pikaia_runs.json"))
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
        print("%s: seed %d, ok %d of %d, paths %s" % (rec["name"], rec["seed"], sum(s["ok"] for s in rec["states"]),
                                                     len(rec["states"]), rec["paths"]))
    print("paths over all shapes: %s" % data["paths"])
    print("wrote %s (%d bytes)" % (a.out, len(text)))


if __name__ == "__main__":
    main()
