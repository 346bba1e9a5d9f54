"""The checks of grad_checks.py on a NumPy stand-in backend (the eigh formulas), where they must pass, and on broken
stand-ins, where they must FAIL - a check that passes a wrong gradient checks nothing.  Also the references against each
other and the differentiated closed form against expm_frechet.  Runs without a GPU."""
import numpy as np
import pytest

import chain_checks as cc
import grad_checks as gc

BROKEN = ("zeros", "time_sign", "reversed", "gamma_diag", "no_h0_diag", "no_h0_offdiag")


@pytest.mark.parametrize("N", [2, 5, 7])
def test_checks_pass_on_the_stand_in(N):
    be = gc.StandIn()
    worst = gc.Worst()
    gc.check_deloc_grad(be, N, worst)
    gc.check_hard_inputs(be, N, worst)
    gc.check_closed_form_grad(be, max(N, 3), worst)
    gc.check_mean_and_shared(be, N)
    assert "deloc" in str(worst)


@pytest.mark.parametrize("broken", BROKEN)
def test_deloc_check_fails_on_a_broken_gradient(broken):
    with pytest.raises(AssertionError):
        gc.check_deloc_grad(gc.StandIn(broken), 7)


@pytest.mark.parametrize("broken", ("zeros", "reversed", "gamma_diag"))
def test_closed_form_check_fails_on_a_broken_gradient(broken):
    with pytest.raises(AssertionError):
        gc.check_closed_form_grad(gc.StandIn(broken), 7)


@pytest.mark.parametrize("N", [2, 5])
def test_generated_draws_checks_pass_on_the_stand_in(N):
    be = gc.StandIn()
    worst = gc.Worst()
    gc.check_static_grad_philox(be, N, worst=worst)
    gc.check_far_offsets_grad_philox(be, N, worst=worst)
    for K in (4096, 4097, 8193):
        gc.check_long_rows_grad_philox(be, N, K)
    assert "static" in str(worst) and "far offset" in str(worst)


@pytest.mark.parametrize("N", [2, 3, 5, 7, 9, 10, 12])
def test_static_cases_have_teeth_for_every_n(N):
    """the guards of check_static_grad_philox (the static terms move F, the gradient is not tiny) hold on the reference"""
    gc.check_static_grad_philox(gc.StandIn(), N, identity=False, reference=False)


@pytest.mark.parametrize("broken", ("no_h0_diag", "no_h0_offdiag", "philox_no_h0_offdiag"))
def test_static_reference_check_fails_on_a_dropped_static_term(broken):
    with pytest.raises(AssertionError, match="static") as e:
        gc.check_static_grad_philox(gc.StandIn(broken), 5, identity=False)
    print(broken, "->", e.value)


def test_static_identity_check_fails_when_only_the_generated_draws_route_drops_the_couplings():
    with pytest.raises(AssertionError, match="differs in") as e:
        gc.check_static_grad_philox(gc.StandIn("philox_no_h0_offdiag"), 5, reference=False)
    print(e.value)
    gc.check_static_grad_philox(gc.StandIn("no_h0_offdiag"), 5, reference=False)      # both routes wrong alike: the reference's job


def test_far_offset_check_fails_on_a_lost_counter_carry():
    with pytest.raises(AssertionError, match="far offset") as e:
        gc.check_far_offsets_grad_philox(gc.StandIn("lost_carry"), 5)
    print(e.value)


@pytest.mark.parametrize("K", (4097, 8193))
def test_long_rows_check_fails_on_row_sums_that_stop_after_64_tiles(K):
    with pytest.raises(AssertionError, match="long rows") as e:
        gc.check_long_rows_grad_philox(gc.StandIn("mean_64_tiles"), 5, K)
    print(e.value)
    gc.check_long_rows_grad_philox(gc.StandIn("mean_64_tiles"), 5, 4096)              # every lane has one tile: nothing to lose


def test_hard_inputs_check_fails_on_a_dropped_time_sign():
    """the mirror-symmetric controller of the hard inputs has a negative time entry"""
    with pytest.raises(AssertionError):
        gc.check_hard_inputs(gc.StandIn("time_sign"), 5)


def test_mean_check_fails_on_a_wrong_mean():
    class WrongMean(gc.StandIn):
        def mc_fidelity_grad(self, *a, **k):
            res = super().mc_fidelity_grad(*a, **k)
            if "mean" in res:
                res["mean"] = res["mean"] * (1 + 1e-9)
            return res
    with pytest.raises(AssertionError):
        gc.check_mean_and_shared(WrongMean(), 5)


def test_teeth_refuse_localised_controllers():
    """uniform random biases U(-10, 10) give gradients of ~1e-6: such a workload cannot tell a wrong kernel from a right one"""
    rng = np.random.default_rng(3)
    N = 7
    ctrl = np.empty((4, N + 1))
    ctrl[:, :N] = rng.uniform(-10, 10, (4, N))
    ctrl[:, N] = rng.uniform(2, 30, 4)
    _, G = gc.grad_eigh(ctrl, 0.05 * rng.standard_normal((4, 50, N, 3)), N, 0, N - 1)
    with pytest.raises(AssertionError):
        gc.assert_grad_teeth(G)


@pytest.mark.parametrize("N", [3, 6])
def test_eigh_formulas_against_frechet(N):
    rng = np.random.default_rng(40 + N)
    ctrl = cc.deloc_ctrl(rng, 3, N, 0.5)
    ctrl[1, N] *= -1
    draws = 0.05 * rng.standard_normal((3, 6, N, 3))
    for (a, b) in gc.grad_pairs(N):
        F1, G1 = gc.grad_eigh(ctrl, draws, N, a, b)
        F2, G2 = gc.grad_frechet(ctrl, draws, N, a, b)
        assert np.abs(F1 - F2).max() < 1e-12
        gc.compare_grad(G1, G2, 0.05 * gc.grad_bars(ctrl, draws, N), (N, a, b))      # the references: a twentieth of the bar


@pytest.mark.parametrize("N", [3, 7, 12])
def test_closed_form_against_frechet(N):
    """d/dT and d/dg of the spin-j closed form against expm_frechet on the dense matrix"""
    ctrl = cc.closed_form_ctrl(N, cc.CF_GS, cc.CF_TS[1::4])
    off = cc.closed_form_offdiag(N)
    draws = np.zeros((ctrl.shape[0], 1, N, 3))
    coef = (N - 1) / 2 - np.arange(N)
    big = 0.0
    for a, b in ((0, N - 1), (N - 1, 1), (0, 0)):
        _, G = gc.grad_frechet(ctrl, draws, N, a, b, None, off)
        dT, dg = gc.closed_form_grad(N, ctrl, a, b)
        assert np.abs(G[:, 0, N] - dT).max() < 1e-12
        assert np.abs(G[:, 0, :N] @ coef - dg).max() < 1e-11
        big = max(big, np.abs(dg).max())
    assert big > 0.1
