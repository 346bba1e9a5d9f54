"""The checks of tests/lbfgs_checks.py have teeth: they pass on `lbfgs.LBFGS` (the definition), and each broken stand-in - the
definition with one defect - fails the check that is there for it.  The known answer (perfect transfer 0 -> 2 of the 3-chain,
gradient from a NumPy eigendecomposition) is checked on the definition too."""
import numpy as np
import pytest

import lbfgs_checks as lc

lbfgs = lc.lbfgs


@pytest.mark.parametrize("name", lc.ALL_CHECKS)
def test_definition_passes(name):
    lc.run_check(name, lc.definition)


def test_known_answer_on_the_definition():
    lc.check_known_answer(lc.definition)


def test_chain3_gradient_is_the_derivative():
    """the analytic gradient behind the known answer against central differences"""
    x = lc.known_answer_start(4, seed=3) + 0.3
    f, g = lc.chain3_one_minus_fidelity(x)
    for i in range(4):
        h = np.zeros(4)
        h[i] = 1e-6
        num = (lc.chain3_one_minus_fidelity(x + h)[0] - lc.chain3_one_minus_fidelity(x - h)[0]) / 2e-6
        assert np.abs(num - g[:, i]).max() <= 1e-8


class _Broken(lbfgs.LBFGS):
    defect = None

    def init(self, x0, mask=None):
        super().init(x0, mask)
        if self.defect == "no_mask":
            self.mask = np.ones_like(self.mask)
        if self.defect == "nan_start_runs":                 # a NaN start row waits for its first value like the others
            self.status = np.zeros_like(self.status)
        return self

    def advance(self, ft, gt):
        done = self.status != 0
        super().advance(ft, gt)
        if self.defect == "ring_never_wraps":               # every pair lands in slot 0
            self.head = np.zeros_like(self.head)
        if self.defect == "done_rows_move":                 # a done row keeps a finite trial point
            self.trial = np.where((self.status != 0)[:, None], self.x, self.trial)
        if self.defect == "done_rows_count":                # ... or keeps counting
            self.evals = self.evals + done
        return self


def broken(defect, **override):
    def factory(x0, mask=None, **params):
        params.update(override)
        mc = _Broken(**params)
        mc.defect = defect
        return mc.init(x0, mask)
    return factory


@pytest.mark.parametrize("check, factory", [
    ("mask", broken("no_mask")),
    ("ring_wraps", broken("ring_never_wraps")),
    ("frozen", broken("done_rows_move")),
    ("frozen", broken("done_rows_count")),
    ("quadratic", broken("done_rows_move")),
    ("wrong_sign", broken(None, maxback=10 ** 6)),          # never gives up
    ("rosenbrock", broken(None, c1=1e-300, maxback=0)),     # a line search that cannot backtrack
    ("nan_start", broken("nan_start_runs")),
], ids=["no_mask", "ring_never_wraps", "done_rows_move", "done_rows_count", "trial_not_nan", "never_gives_up", "no_backtracking",
        "nan_start_runs"])
def test_broken_stand_in_fails(check, factory):
    with pytest.raises(AssertionError):
        lc.run_check(check, factory)


def test_objective_kinds():
    """`lbfgs.objective`: kind 2 is `noise.moments_from_sums`, operation for operation (floor rule included)"""
    import importlib
    noise = importlib.import_module("code-robchar_amd.noise")
    mean, moment = lc.sample_rows(6, 3)(np.random.default_rng(0).standard_normal((9, 6)))
    moment[3, 0] = mean[3, 0] ** 2                          # a row on the variance floor
    mo = noise.moments_from_sums(mean, moment)
    f, g = lbfgs.objective("one_minus_plus_std", mean, moment, 0.75)
    assert mo["std"][3] == 0.0 and np.array_equal(f, (1.0 - mo["fav"]) + 0.75 * mo["std"])
    assert np.array_equal(g, -mo["grad_fav"] + 0.75 * mo["grad_std"])
    f, g = lbfgs.objective("one_minus", mean)
    assert np.array_equal(f, 1.0 - mean[:, 0]) and np.array_equal(g, -mean[:, 1:])
    f, g = lbfgs.objective("raw", mean)
    assert np.array_equal(f, mean[:, 0]) and np.array_equal(g, mean[:, 1:])


def test_state_layout():
    n, m, C = 7, 3, 4
    mc = lc.definition(np.zeros((C, n)) + 0.1, None, m=m)
    off = lbfgs.field_offsets(n, m)
    arr = mc.state_array()
    assert arr.shape == (lbfgs.state_fields(n, m), C) == (off["len"], C)
    assert (arr[off["first"]] == 1.0).all() and (arr[off["mask"]:off["mask"] + n] == 1.0).all() and off["mask"] + n == off["len"]
