"""The checks of grad_times_checks.py pass on the NumPy stand-in of `backend.mc_fidelity_grad_times_philox` and fail on every
broken stand-in; the teeth guards hold on the reference for the oracle workload of times_checks.py - runs without a GPU."""
import numpy as np
import pytest

import grad_checks as gc
import grad_times_checks as gt
import times_checks as tc


def test_checks_pass_on_the_stand_in():
    be = gt.StandIn()
    for N in (3, 10):
        a, b = 0, N - 1
        gt.check_bits_against_single_time(be, N, a, b, K=12)
        gt.check_unit_grid(be, N, a, b, K=12)
        gt.check_means_and_moments(be, N, a, b, K=12)
        gt.check_reference(be, N, a, b, K=12, guard=False)
        gt.check_cross_times_kernel(be, N, a, b, K=12)
    gt.check_semantics(be, 3, K=6)


def _fails(check, be, *args, **kw):
    with pytest.raises(AssertionError):
        check(be, *args, **kw)


@pytest.mark.parametrize("broken", gt.StandIn.BROKEN)
def test_checks_fail_on_every_broken_stand_in(broken):
    be = gt.StandIn(broken)
    N = 10 if broken == "W summed over the passes" else 3
    a, b = 0, N - 1
    if broken == "moments with F(T)":
        _fails(gt.check_reference, be, N, a, b, K=12, guard=False)        # (the per-sample outputs are right: only the moments see it)
        gt.check_bits_against_single_time(be, N, a, b, K=12)
        return
    _fails(gt.check_reference, be, N, a, b, K=12, guard=False)
    _fails(gt.check_bits_against_single_time, be, N, a, b, K=12)
    if broken == "W summed over the passes":
        _fails(gt.check_cross_times_kernel, be, N, a, b, K=12)


def test_moments_with_the_wrong_fidelity_fail_the_host_sums():
    """check 3 forms the moments from the call's own W: a stand-in whose moments use F(T) fails it"""
    _fails(gt.check_means_and_moments, gt.StandIn("moments with F(T)"), 3, 0, 2, K=12)


def test_no_sign_fails_the_semantics_check():
    _fails(gt.check_semantics, gt.StandIn("no sgn(u)"), 3, K=6)


@pytest.mark.parametrize("N,a,b", [p for p in tc.PAIRS if p[0] <= 12])
def test_teeth_guards_hold_on_the_oracle_workload(N, a, b):
    """the measured values behind MIN_BIAS_TEETH / MIN_TIME_TEETH: the oracle workload's controllers with N(0, 0.05^2) draws"""
    ctrl, draws, _ = tc.oracle_workload(N, a, b)
    _, G, _, _, G0 = gt.reference(ctrl, draws, N, a, b, gt.TSCALE, gt.TSHIFT, gt.WEIGHTS)
    tb, tt = gt.assert_teeth(G, G0, gt.WEIGHTS, (N, a, b))
    print(f"teeth N = {N} {a} -> {b}: bias {tb:.4f} time {tt:.4f}")


@pytest.mark.parametrize("N,a,b", [p for p in tc.PAIRS if p[0] <= 12])
def test_teeth_guards_hold_under_the_generated_draws(N, a, b):
    """... and on the same controllers under the draws the entry generates (what the GPU test asserts them on), K = 70 and 130"""
    ctrl = gt.guarded_ctrl(N, a, b)
    for (K, shared) in ((70, False), (130, True)):
        _, G, _, _, G0 = gt.reference(ctrl, gt.draws_of(ctrl, K, N, 0, shared), N, a, b, gt.TSCALE, gt.TSHIFT, gt.WEIGHTS)
        tb, tt = gt.assert_teeth(G, G0, gt.WEIGHTS, (N, a, b, K))
        print(f"teeth N = {N} {a} -> {b}, K = {K}: bias {tb:.4f} time {tt:.4f}")


def test_the_guard_catches_a_backend_that_ignores_the_grid():
    """on the guarded controllers the reference moves by more than the guards, so `check_reference` fails such a backend by far"""
    N, a, b = 3, 0, 2
    _fails(gt.check_reference, gt.StandIn("grid ignored"), N, a, b, K=12, ctrl=gt.guarded_ctrl(N, a, b))
    gt.check_reference(gt.StandIn(), N, a, b, K=70, ctrl=gt.guarded_ctrl(N, a, b))


def test_signed_times_are_the_readout_times():
    T = np.array([3.7, -2.2, 0.0, 41.123456789])
    assert np.array_equal(np.abs(gt.signed_times(T, gt.TSCALE, gt.TSHIFT)), tc.times_of(T, gt.TSCALE, gt.TSHIFT))
    assert (gt.signed_times(T, gt.TSCALE, gt.TSHIFT) < 0).any()
