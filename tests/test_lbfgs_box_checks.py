"""The checks of tests/lbfgs_box_checks.py have teeth: they pass on the boxed `lbfgs.LBFGS` (the definition), and each broken
stand-in fails the check that is there for it: one that ignores the bounds, one that clips the trial point but keeps no active
set, one that freezes every variable that touches a bound, and one that tests max |g_i| for status 1.  Without bounds the
definition still gives the bits of a run recorded before the box existed."""
import os

import numpy as np
import pytest

import lbfgs_box_checks as bc
import lbfgs_checks as lc

lbfgs = lc.lbfgs
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lbfgs_unbounded_run.npz")


@pytest.mark.parametrize("name", bc.ALL_CHECKS)
def test_definition_passes(name):
    bc.run_check(name, bc.definition)


def ignores_bounds(x0, mask=None, lo=None, hi=None, **params):
    return lbfgs.LBFGS(**params).init(x0, mask)


class _ClipOnly(lbfgs.LBFGS):
    """the unbounded machine with its start and every trial point clipped into the box: no active set, the unbounded accept rule"""

    def init(self, x0, mask=None, lo=None, hi=None):
        C, n = np.shape(x0)
        self.blo, self.bhi = np.broadcast_to(lo, (C, n)), np.broadcast_to(hi, (C, n))
        return super().init(bc.project(np.asarray(x0, dtype=np.float64), self.blo, self.bhi), mask)

    def advance(self, ft, gt):
        super().advance(ft, gt)
        self.trial = bc.project(self.trial, self.blo, self.bhi)
        return self


class _Freezes(lbfgs.LBFGS):
    """the boxed machine, but a variable that touches a bound never moves again: its gradient is dropped"""

    def advance(self, ft, gt):
        with np.errstate(invalid="ignore"):
            free = (self.trial > self.lo) & (self.trial < self.hi)
        return super().advance(ft, np.where(free | np.isnan(self.trial), gt, 0.0))


class _PlainGradientTest(lbfgs.LBFGS):
    """the boxed machine with max |g_i| <= gtol for status 1"""

    def _stationarity(self):
        return lbfgs._absmax(self.g)


def stand_in(cls):
    return lambda x0, mask=None, lo=None, hi=None, **params: cls(**params).init(x0, mask, lo, hi)


@pytest.mark.parametrize("check, factory", [
    ("invariants", ignores_bounds),
    ("separable", ignores_bounds),
    ("start_rows", ignores_bounds),
    ("bad_bounds", ignores_bounds),
    ("separable", stand_in(_ClipOnly)),
    ("coupled", stand_in(_ClipOnly)),
    ("start_rows", stand_in(_Freezes)),
    ("separable", stand_in(_PlainGradientTest)),
    ("one_sided", stand_in(_PlainGradientTest)),
], ids=["ignores_bounds-invariants", "ignores_bounds-separable", "ignores_bounds-start_rows", "ignores_bounds-bad_bounds",
        "clip_only-separable", "clip_only-coupled", "freezes-start_rows", "plain_gradient_test-separable",
        "plain_gradient_test-one_sided"])
def test_broken_stand_in_fails(check, factory):
    with pytest.raises(AssertionError):
        bc.run_check(check, factory)


def test_separable_cost():
    """the separable check is the quick one: a few dozen evaluations"""
    assert bc.check_separable(bc.definition) <= 60


def test_identity_cases_are_not_one_story():
    """the rows of the bit-identity cases hit bounds, reject, reset and finish in different ways"""
    for n, m, kind in ((3, 1, 0), (8, 3, 1), (13, 8, 2), (6, 5, 1)):
        case = bc.identity_case(n, m, kind, C=65)
        print(n, m, kind, case["counters"], sorted(set(case["status"])))
        assert case["counters"]["rejected"] > 0 and case["counters"]["on_bound"] > 0, case["counters"]
        assert len(set(case["status"])) >= 3 and 5 in case["status"], case["status"]
        off = lbfgs.field_offsets(n, m)
        for a, b, state, trial in case["calls"]:
            x = state[off["x"]:off["x"] + n].T
            ok = ~np.isin(np.arange(65), (1, 3, 5))                           # (the NaN start row and the two rows with bad bounds)
            assert (x[ok] >= case["lo"][ok]).all() and (x[ok] <= case["hi"][ok]).all()
    assert sum(bc.identity_case(n, m, kind, C=65)["counters"]["reset"] for n, m, kind in ((8, 3, 1), (13, 8, 2), (6, 5, 1))) > 0


def test_no_bounds_is_the_recorded_unbounded_run():
    """`init(x0, mask)` without bounds: the state and trial bits of a run recorded from lbfgs.py as it was before the box"""
    z = np.load(GOLDEN)
    params = {k[len("param_"):]: z[k].item() for k in z.files if k.startswith("param_")}
    mc = lbfgs.LBFGS(m=int(z["m"]), **params).init(z["x0"], z["mask"])
    assert not mc.box
    assert np.array_equal(mc.state_array(), z["init_state"], equal_nan=True) and np.array_equal(mc.trial, z["init_trial"], equal_nan=True)
    assert len(z["a"]) == 25
    for call in range(len(z["a"])):
        with np.errstate(all="ignore"):
            mc.advance(*lbfgs.objective(int(z["kind"]), z["a"][call], z["b"][call], float(z["lam"])))
        assert np.array_equal(mc.state_array(), z["state"][call], equal_nan=True), call
        assert np.array_equal(mc.trial, z["trial"][call], equal_nan=True), call
    assert len(set(mc.status)) >= 3


def test_infinite_box_reaches_the_unbounded_minimiser():
    """lo = -inf, hi = +inf everywhere: no projection ever acts and no variable is ever active, so the boxed machine converges to
    the same minimiser as the unbounded one (its accept rule reads g.s, not (c1 t) g.d: equal to rounding, not bit for bit)"""
    fun, xs, A = lc.quadratic(6, seed=6)
    x0 = xs + np.random.default_rng(1).standard_normal((5, 6))
    mc = bc.definition(x0, None, -np.inf, np.inf, gtol=1e-9, maxiter=200)
    lc.drive(mc, fun, 400)
    assert (mc.status == 1).all() and np.abs(mc.x - xs).max() <= np.sqrt(6) * 1e-9


def test_layout_unchanged():
    for n, m in ((3, 1), (8, 5), (13, 8)):
        mc = bc.definition(np.zeros((4, n)), None, -1.0, 1.0, m=m)
        assert mc.state_array().shape == (lbfgs.state_fields(n, m), 4) == (4 * n + 2 * m * n + m + 11, 4)
