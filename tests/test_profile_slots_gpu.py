"""Every launch in its own slot of get("profile"): the launch counts per slot after two iterate()
calls, per engine whose launches go through Engine::timed(), with a built-in objective and with a
Python callable (the spans differ where the host evaluates).

The layout of "profile" is KernelTimer::report's, [ms0, calls0, ms1, calls1, ...]; the times are not
asserted.  TABLE was filled by running launch_counts() below on an MI355X with the library as it
was BEFORE the engines' hand-written timer spans became timed() calls, so a launch that moved to
another slot, or a span that was lost or doubled, shows as a difference.  Shapes are the smallest
the classes accept: n = 4, two populations, eight individuals (HEES and xNES size themselves).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, NP, POPS, SEED = 4, 8, 2, 1234
LOWER, UPPER = -5. * np.ones(N), 5. * np.ones(N)
GUESS = np.random.default_rng(5).uniform(-3., 3., N * POPS)

K = dict(seed=SEED, populations=POPS)
CASES = {
    "CMAES": lambda hip: hip.CMAES(100000, 1e-12, NP, **K),
    "ActiveCMAES": lambda hip: hip.ActiveCMAES(100000, 1e-12, NP, **K),
    "SepCMAES": lambda hip: hip.SepCMAES(100000, 1e-12, NP, **K),
    "CholeskyCMAES": lambda hip: hip.CholeskyCMAES(100000, 1e-12, 1e-12, NP, **K),
    "LmCMAES": lambda hip: hip.LmCMAES(100000, 1e-12, NP, **K),
    "JADE": lambda hip: hip.JADE(100000, NP, 1e-12, **K),
    "SHADE": lambda hip: hip.SHADE(100000, NP, 1e-12, **K),
    "SANSDE": lambda hip: hip.SANSDE(100000, NP, 1e-12, **K),
    "CSO": lambda hip: hip.CSO(100000, 1e-12, NP, pcompete=2, **K),
    "CCPSO": lambda hip: hip.CCPSO(100000, 1e-12, NP, [2], **K),
    "APSO": lambda hip: hip.APSO(100000, 1e-12, NP, **K),
    "JAYA": lambda hip: hip.JAYA(100000, 1e-12, NP, 2, **K),
    "DSA": lambda hip: hip.DSA(100000, 1e-12, 1e-12, NP, **K),
    "HEES": lambda hip: hip.HEES(100000, 1e-12, **K),
    "xNES": lambda hip: hip.xNES(100000, 1e-12, **K),
    "AMALGAM": lambda hip: hip.AMALGAM(100000, 1e-12, 1e-12, np=NP, noparam=False, print=False, **K),
    "SpiralSearch": lambda hip: hip.SpiralSearch(100000, 1e-12, np=NP, **K),
    "NSHS": lambda hip: hip.NSHS(100000, NP, **K),
}

# (class, objective) -> launches per slot after initialize(), set("profile") and two iterate() calls
TABLE = {
    ("CMAES", "builtin"): (2, 2, 0, 2, 2, 2, 2, 2, 2),
    ("CMAES", "callable"): (2, 2, 0, 2, 2, 2, 2, 2, 2),
    ("ActiveCMAES", "builtin"): (2, 2, 0, 2, 2, 2, 2, 2, 2),
    ("ActiveCMAES", "callable"): (2, 2, 0, 2, 2, 2, 2, 2, 2),
    ("SepCMAES", "builtin"): (2, 2, 0, 2, 2, 0, 0, 0, 2),
    ("SepCMAES", "callable"): (2, 2, 0, 2, 2, 0, 0, 0, 2),
    ("CholeskyCMAES", "builtin"): (2, 2, 0, 2, 2, 2, 0, 0, 2),
    ("CholeskyCMAES", "callable"): (2, 2, 0, 2, 2, 2, 0, 0, 2),
    ("LmCMAES", "builtin"): (2, 2, 2, 2, 2, 2),
    ("LmCMAES", "callable"): (2, 2, 2, 2, 2, 2),
    ("JADE", "builtin"): (2, 2, 2, 2, 2, 0),
    ("JADE", "callable"): (2, 2, 2, 2, 2, 2),
    ("SHADE", "builtin"): (2, 2, 2, 2, 2, 0),
    ("SHADE", "callable"): (2, 2, 2, 2, 2, 2),
    ("SANSDE", "builtin"): (2, 2, 0, 2, 2, 0),
    ("SANSDE", "callable"): (2, 2, 0, 2, 2, 2),
    ("CSO", "builtin"): (2, 2, 2, 2, 2),
    ("CSO", "callable"): (2, 2, 2, 2, 2),
    ("CCPSO", "builtin"): (2, 2, 2, 2, 2),
    ("CCPSO", "callable"): (2, 2, 2, 2, 2),
    ("APSO", "builtin"): (2, 2, 2, 2, 2),
    ("APSO", "callable"): (2, 2, 2, 2, 2),
    ("JAYA", "builtin"): (2, 2, 2),
    ("JAYA", "callable"): (2, 2, 2),
    ("DSA", "builtin"): (2, 2, 2, 2),
    ("DSA", "callable"): (2, 2, 2, 2),
    ("HEES", "builtin"): (2, 2, 2, 2, 2, 2, 2),
    ("HEES", "callable"): (2, 2, 2, 2, 2, 2, 2),
    ("xNES", "builtin"): (2, 2, 2, 2, 2),
    ("xNES", "callable"): (2, 2, 2, 2, 2),
    ("AMALGAM", "builtin"): (2, 2, 2, 2, 2, 2, 2),
    ("AMALGAM", "callable"): (2, 2, 2, 2, 2, 2, 2),
    ("SpiralSearch", "builtin"): (2, 2, 2, 2),
    ("SpiralSearch", "callable"): (2, 2, 0, 2),
    ("NSHS", "builtin"): (0, 2, 2, 2, 0),
    ("NSHS", "callable"): (0, 2, 0, 2, 0),
}


def launch_counts(hip, name, objective):
    f = hip.objectives.sphere if objective == "builtin" else (lambda x: float(np.sum(x * x)))
    g = CASES[name](hip)
    g.initialize(f, LOWER, UPPER, GUESS)
    g.set_state("profile", [1.])
    g.iterate()
    g.iterate()
    return tuple(int(c) for c in g.get_state("profile").reshape(-1, 2)[:, 1])


@pytest.mark.parametrize("objective", ["builtin", "callable"])
@pytest.mark.parametrize("name", list(CASES))
def test_launches_per_slot(hip, name, objective):
    got = launch_counts(hip, name, objective)
    print(name, objective, got)
    assert got == TABLE[(name, objective)]
