"""CPU: tests/lm_model.py against the recorded reference (tests/golden/lm_runs.json).

The reference form of the model reproduces every recorded state of "steps" bit for bit, given the
recorded draws.  The device form differs from it in the order of the dot products over n, of the
built-in objectives' sums and in the sigma rule's numerator: its deviation is rounding only.  The
test prints the largest deviation relative to the largest entry of the key, per run, key and
generation; the largest figure over all of them, DEVICE_FORM_DEVIATION, is what the bounds of
tests/test_lm_golden_gpu.py are set from.  Measured: 7.3e-15 (n16_l12_rad, generation 17, s); the
test holds the device form to 1e-12, some 1e4 roundings of a double and a tenth of the tightest
bound the GPU test uses."""
import base64

import numpy as np
import pytest

import lm_model as lm
from _golden import load

GOLD = load("lm_runs.json")
STEPS = {s["name"]: s for s in GOLD["steps"]}
INT_KEYS = ("fit_idx", "jarr", "larr", "memlen", "it", "fev", "flag")
KEYS = ("arx", "fit_val", "fit_idx", "xmean", "sigma", "pc", "s", "memlen", "jarr", "larr", "b", "d", "pcmat",
        "vmat", "fp", "it", "fev", "flag")
DEVICE_FORM_BOUND = 1e-12


def unpack(s):
    """an array of the fixture: base64 of little-endian IEEE doubles"""
    return np.frombuffer(base64.b64decode(s), dtype="<f8").astype(np.float64)


def draws_of(rec, st):
    """a generation's table [ceil(lambda / 2)][n + 1]: z (a Rademacher row is a string of + and -), g"""
    half, n = (rec["lambda"] + 1) // 2, rec["n"]
    if rec["rademacher"]:
        z = np.array([[1. if c == "+" else -1. for c in row] for row in st["z"]])
    else:
        z = unpack(st["z"]).reshape(half, n)
    return np.concatenate([z, unpack(st["g"])[:, None]], axis=1)


def recorded(st, key, n):
    v = st[key]
    if key in ("memlen", "it", "fev", "flag"):
        return np.array([float(v)])
    if key in ("fit_idx", "jarr", "larr"):
        return np.array(v, float)
    return unpack(v)


def model_of(rec, device):
    box = rec["box"]
    m = lm.LmModel(rec["mfev"], rec["tol"], rec["lambda"], 0, rec["sigma0"], bool(rec["bound"]),
                   bool(rec["usenew"]), device=device)
    n = rec["n"]
    m.init(rec["objective"], -box * np.ones(n), box * np.ones(n), unpack(rec["guess"]))
    return m


def trimmed(state, key, memlen, n):
    v = state[key]
    return v[:memlen * n] if key in ("pcmat", "vmat") else v


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("name", list(STEPS))
def test_reference_form_reproduces_the_recorded_states_bit_for_bit(name):
    rec = STEPS[name]
    m, n = model_of(rec, False), rec["n"]
    assert (m.m, m.t, m.nsteps) == (rec["memory"], rec["t"], rec["nsteps"])
    seen = set()
    for st in rec["states"]:
        m.generation(draws_of(rec, st))
        assert m.it == st["it"]
        if st["gen"] not in rec["recorded"]:
            continue
        seen.add(m.last_branch)
        got = m.state()
        for k in KEYS:
            want = recorded(st, k, n)
            have = trimmed(got, k, st["memlen"], n)
            assert have.shape == want.shape, (k, st["gen"])
            assert have.tobytes() == want.tobytes(), (k, st["gen"], have[have != want][:4], want[have != want][:4])
    assert seen - {None}, name


def test_every_branch_of_the_slot_list_is_in_a_recorded_generation():
    seen = set()
    for rec in GOLD["steps"]:
        m = model_of(rec, False)
        for st in rec["states"]:
            m.generation(draws_of(rec, st))
            if st["gen"] in rec["recorded"]:
                seen.add(m.last_branch)
    assert {"fill", "remove", "drop0"} <= seen


def device_form_deviation(verbose=False):
    worst = (0., None)
    for rec in GOLD["steps"]:
        m, n = model_of(rec, True), rec["n"]
        for st in rec["states"]:
            m.generation(draws_of(rec, st))
            if st["gen"] not in rec["recorded"]:
                continue
            got = m.state()
            for k in KEYS:
                want, have = recorded(st, k, n), trimmed(got, k, st["memlen"], n)
                if k in INT_KEYS:
                    assert np.array_equal(have, want), (rec["name"], k, st["gen"])
                    continue
                dev = rel(have, want)
                if verbose:
                    print("%-16s gen %2d %-8s %.3e" % (rec["name"], st["gen"], k, dev))
                if dev > worst[0]:
                    worst = (dev, (rec["name"], st["gen"], k))
    return worst


def test_device_form_deviates_by_rounding_only():
    dev, where = device_form_deviation(verbose=True)
    print("largest deviation of the device form: %.3e at %s" % (dev, where))
    assert dev < DEVICE_FORM_BOUND, where


def test_tie_free_fixture():
    """no rank of the fixture rests on a tie: neighbours of every recorded generation's ranking
    differ by more than 1e-9 relative"""
    for rec in GOLD["steps"]:
        for st in rec["states"]:
            if st["gen"] in rec["recorded"]:
                f = unpack(st["fit_val"])
                pooled = np.sort(np.concatenate([f, unpack(st["fp"])])) if st["it"] > 1 else f
                for v in (f, pooled):
                    gap = np.diff(v) / np.maximum(np.abs(v[1:]), np.abs(v[:-1]))
                    assert gap.min() > 1e-9, (rec["name"], st["gen"])


def test_stop_tests_of_the_model():
    """each of the four stop tests from the model's own state (the fixture's "runs" reach all four
    in the reference as well)"""
    m = lm.LmModel(24, 1e-8, 12)
    m.init("sphere", -np.ones(4), np.ones(4), np.zeros(4))
    assert m.flag() == 0
    m.it = 2
    assert m.flag() == lm.FLAG_MAXITER
    m.it, m.sigma = 1, 9e-17
    assert m.flag() == lm.FLAG_SIGMA
    m.sigma, m.it, m.fbest, m.fworst = 1., m.hlen, 1., 1. + 1e-9
    m.mit = 10 ** 6
    assert m.flag() == lm.FLAG_TOLHISTFUN
    m.tol, m.hcount, m.hbuf = 0., 4, 3
    m.hbest[:4], m.hkth[:4] = [1., 2., 3., 4.], [1., 2., 0., 0.]
    assert m.flag() == lm.FLAG_EQUALFUNVALS
    m.hkth[:4] = [1., 0., 0., 0.]
    assert m.flag() == 0
    kinds = {r["stop"] for r in GOLD["runs"]["stops"]}
    assert kinds == {"MaxIter", "TolHistFun", "EqualFunVals", "SigmaTooSmall"}


def test_device_dot_is_the_sum():
    rng = np.random.default_rng(5)
    for n in (1, 63, 64, 65, 257, 1000, 4096):
        a, b = rng.standard_normal(n), rng.standard_normal(n)
        exact = float(np.sum(a.astype(np.longdouble) * b.astype(np.longdouble)))
        scale = float(np.abs(a * b).sum())
        assert abs(lm.dev_dot(a, b) - exact) <= 64 * np.finfo(float).eps * scale
        assert abs(lm.seq_dot(a, b) - exact) <= n * np.finfo(float).eps * scale
