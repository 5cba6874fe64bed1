"""GPU: the energies BasinHopping's hop kernel evaluates (bh_collect, with the minimiser's own device value
function) lie inside the bound every built-in form is held to."""
import pytest

import objective_reference as R
import test_rosenbrock_forms_gpu  # noqa: F401  (its row: the table is complete only with every row registered)
import test_objective_forms_gpu as T


def _make(kind):
    def make(hip, n):
        inner = hip.NelderMead(300, 1e-8, 0.5, seed=3) if kind == "nm" else hip.Rosenbrock(300, 1e-6, 0.5, repair=True, seed=3)
        return hip.BasinHopping(inner, hip.BasinHopping_StepStrategy(0.1), False, 4, seed=3)
    return make


# BasinHopping's row in the table of call sites of tests/test_objective_forms_gpu.py, registered at import as the
# rows of the engines before it are.  One form of evaluation whatever n is (eval_row_group<64> over xsol in global
# memory).  The pairs: the incumbent and the best with their energies.
T.SITES["BasinHopping"] = T.Site(_make("nm"), [("x", "energy"), ("xbest", "fbest")], ns=(1, 17, 65, 128))
SITE = T.SITES["BasinHopping"]


def test_the_row_is_in_the_table():
    """(no device)"""
    T.test_the_table_names_every_optimizer_class()
    assert SITE.ns == (1, 17, 65, 128) and SITE.clamp_kw is None and not SITE.extra


@pytest.mark.gpu
@pytest.mark.parametrize("n", SITE.ns)
def test_call_sites_inside_the_bound(hip, n):
    """initialize, two hops, the incumbent and the best with their energies, all ten objectives, both minimisers
    (Rosenbrock under repair: without it a budget exit returns the zero vector)"""
    for kind in ("nm", "rosen"):
        T._hold_site(hip, "BasinHopping", n, R.OBJECTIVES, -5., 5., make=_make(kind))
