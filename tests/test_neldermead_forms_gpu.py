"""NelderMead's row in the table of call sites of tests/test_objective_forms_gpu.py (SITES: one row per optimizer
class, "a new engine cannot arrive without a row"), and the checks that table drives, for that row: every value
the engine exposes next to a point is held to the extended-precision reference of the objective at that point,
for all ten built-in objectives.

The row is registered here, at import, so that the table's own completeness test sees it; the parametrised
tests of that module were generated before, so the cases of this row are generated below.

NelderMead evaluates with one form whatever n is (eval_row_group<64> over a row of the simplex or over the
candidate point, in LDS or in global memory: the same arithmetic).  n = 128 is its limit.  It has no population
argument and never clamps.  The pair: the simplex and its values, "p" / "y".  repair=True: the literal reference
stores a refused outside contraction's pstar with the value of ANOTHER point (nelder_mead.cpp:195-197), which
is no pair."""
import pytest

import objective_reference as R
import test_objective_forms_gpu as T
import test_pikaia_forms_gpu  # noqa: F401  (its row: the table is complete only with every row registered)

T.SITES["NelderMead"] = T.Site(lambda hip, n: hip.NelderMead(T.BUDGET, 0., 1., repair=True, seed=3), [("p", "y")],
                               ns=(1, 17, 65, 128))
SITE = T.SITES["NelderMead"]


def test_the_row_is_in_the_table():
    """(no device)"""
    T.test_the_table_names_every_optimizer_class()
    assert SITE.ns == (1, 17, 65, 128) and SITE.clamp_kw is None and not SITE.extra


@pytest.mark.gpu
@pytest.mark.parametrize("n", SITE.ns)
def test_call_sites_inside_the_bound(hip, n):
    """initialize, two iterations, every exposed (points, values) pair, all ten objectives"""
    T._hold_site(hip, "NelderMead", n, R.OBJECTIVES, -5., 5.)


@pytest.mark.gpu
def test_call_sites_simplex_in_global_memory(hip):
    """the same rows evaluated where lds=False leaves them"""
    T._hold_site(hip, "NelderMead", 65, R.OBJECTIVES, -5., 5.,
                 make=lambda hip, n: hip.NelderMead(T.BUDGET, 0., 1., repair=True, lds=False, seed=3))
