"""The checks of sens_checks.py on the CPU: the two references agree, a correct NumPy stand-in passes every check, and every
broken one fails at least one."""
import numpy as np
import pytest

import chain_checks as cc
import grad_checks as gc
import sens_checks as sc


@pytest.mark.parametrize("N", [2, 3, 5, 7, 12])
def test_references_agree(N):
    rng = np.random.default_rng(40 + N)
    ctrl = cc.deloc_ctrl(rng, 2, N, 0.5)
    ctrl[1, N] = -ctrl[1, N]
    for sigma in (0.05, 0.5):
        draws = sigma * rng.standard_normal((2, 2, N, 3))
        for (a, b) in gc.grad_pairs(N)[:3]:
            F1, S1 = sc.sens_frechet(ctrl, draws, N, a, b)
            F2, S2 = sc.sens_eigh(ctrl, draws, N, a, b)
            assert np.abs(F1 - F2).max() < 1e-13
            assert np.abs(S1 - S2).max() < 1e-12 * max(1.0, np.abs(ctrl[:, N]).max()), (N, sigma, a, b)
    assert np.abs(S2).max() > 1e-2


def test_radial_identity_against_central_difference_in_sigma():
    """row mean of rho = sigma dFbar/dsigma for draws sigma z (the identity the kernel's mean rho rests on)"""
    N, K, sigma, h = 5, 400, 0.05, 1e-4
    rng = np.random.default_rng(9)
    ctrl = cc.deloc_ctrl(rng, 3, N, 0.5)
    z = rng.standard_normal((1, K, N, 3))
    F, S = sc.sens_eigh(ctrl, sigma * z, N, 0, N - 1)
    rho = sc.mean_of(F, sigma * z, S)[:, 1]
    fp = sc.sens_eigh(ctrl, sigma * (1 + h) * z, N, 0, N - 1)[0].mean(axis=1)
    fm = sc.sens_eigh(ctrl, sigma * (1 - h) * z, N, 0, N - 1)[0].mean(axis=1)
    assert np.abs(rho).max() > 1e-3
    assert np.abs((fp - fm) / (2 * h) - rho).max() < 1e-7


@pytest.mark.parametrize("N", [3, 8])
def test_closed_form_dlam_against_central_difference(N):
    ctrl = cc.closed_form_ctrl(N, cc.CF_GS, cc.CF_TS[1:])
    h = 1e-6
    for a in (0, N - 1):
        for b in range(N):
            fd = (cc.closed_form_fid(N, ctrl, a, b, lam=1 + h) - cc.closed_form_fid(N, ctrl, a, b, lam=1 - h)) / (2 * h)
            assert np.abs(fd - sc.closed_form_dlam(N, ctrl, a, b)).max() < 1e-8


def _all_checks(be, N):
    sc.check_deloc_sens(be, N)
    sc.check_closed_form_sens(be, N)
    sc.check_hard_sens(be, N)
    sc.check_consistency(be, N)


@pytest.mark.parametrize("N", [2, 5, 12])
def test_stand_in_passes(N):
    _all_checks(sc.StandIn(), N)


@pytest.mark.parametrize("N", range(2, 13))
def test_reference_has_teeth_for_every_n(N):
    """the teeth guards of check_deloc_sens hold on the reference for every N the kernel is built for"""
    sc.check_deloc_sens(sc.StandIn(), N)


@pytest.mark.parametrize("broken", sc.BROKEN)
def test_broken_stand_ins_fail(broken):
    with pytest.raises(AssertionError):
        _all_checks(sc.StandIn(broken), 5)
