"""PIKAIA's row in the table of call sites of tests/test_objective_forms_gpu.py (SITES: one row per optimizer
class, "a new engine cannot arrive without a row"), and the checks that table drives, for that row: every value
the engine exposes next to a point is held to the extended-precision reference of the objective at that point,
for all ten built-in objectives.

The row is registered here, at import, so that the table's own completeness test sees it; the parametrised
tests of that module were generated before, so the cases of this row are generated below.

PIKAIA evaluates with one kernel form whatever n is (eval_row_group<64> over the row in global memory, in the
breeding kernel and, for the elite row, in pikaia_newpop): no extra cases.  np = 2 is the smallest population
(even, two parents that differ).  It maps the unit cube onto the box and never clamps: u < 1, so no coordinate
lies on the upper bound and the lower bound takes u = 0 exactly, one draw in 10^nd.  Pairs: the offspring of the
last generation with their values (after a generation they are the population, "x"), and the best ever."""
import pytest

import objective_reference as R
import test_objective_forms_gpu as T

T.SITES["PIKAIA"] = T.Site(lambda hip, n: hip.PIKAIA(2, T.BUDGET, 6, ielite=1, seed=3),
                           [("new_x", "new_f"), ("xbest", "fbest")])
SITE = T.SITES["PIKAIA"]


def test_the_row_is_in_the_table():
    """(no device)"""
    T.test_the_table_names_every_optimizer_class()
    assert SITE.ns == (1, 17, 65, 130) and SITE.clamp_kw is None and not SITE.extra


@pytest.mark.gpu
@pytest.mark.parametrize("n", SITE.ns)
def test_call_sites_inside_the_bound(hip, n):
    """initialize, two iterations, every exposed (points, values) pair, all ten objectives"""
    T._hold_site(hip, "PIKAIA", n, R.OBJECTIVES, -5., 5.)
