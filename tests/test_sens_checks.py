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


@pytest.mark.parametrize("N", [3, 5])
def test_generated_draws_checks_pass_on_the_stand_in(N):
    be = sc.StandIn()
    worst = gc.Worst()
    sc.check_static_sens_philox(be, N, worst=worst)
    sc.check_cut_bond_sens_philox(be, N, worst=worst)
    sc.check_far_offsets_sens_philox(be, N, worst=worst)
    for K in (4096, 4097, 8193):
        sc.check_long_rows_sens_philox(be, N, K)
    sc.check_long_rows_sens(be, N, 4097)
    assert all(k in str(worst) for k in ("static", "cut bond", "far offset"))


@pytest.mark.parametrize("N", [2, 3, 5, 7, 10, 12])
def test_static_cases_have_teeth(N):
    """the reference-only guards of the static-term check hold at every N the GPU tests run it at"""
    sc.check_static_sens_philox(sc.StandIn(), N, identity=False, reference=False)


@pytest.mark.parametrize("N", [3, 7, 11])
def test_cut_bond_check_passes_on_the_stand_in(N):
    sc.check_cut_bond_sens_philox(sc.StandIn(), N)


@pytest.mark.parametrize("broken", ("no_h0_diag", "no_h0_offdiag", "re_g1", "philox_no_h0_offdiag"))
def test_static_reference_check_fails_on_wrong_static_terms(broken):
    with pytest.raises(AssertionError, match="static") as e:
        sc.check_static_sens_philox(sc.StandIn(broken), 5, identity=False)
    print(broken, "->", e.value)


def test_static_identity_check_fails_when_only_the_generated_draws_route_drops_the_couplings():
    with pytest.raises(AssertionError, match="differs in") as e:
        sc.check_static_sens_philox(sc.StandIn("philox_no_h0_offdiag"), 5, reference=False)
    print(e.value)


@pytest.mark.parametrize("broken", ("re_g1", "no_h0_offdiag", "no_phase"))
def test_cut_bond_check_fails(broken):
    """re = g1 at the cut bond of the sigma = 0 row is 0 / 0; without h0_offdiag the chain is not cut; dF/dr without re / r is 0 / 0"""
    with pytest.raises(AssertionError, match="cut bond") as e:
        sc.check_cut_bond_sens_philox(sc.StandIn(broken), 7)
    print(broken, "->", e.value)


def test_far_offset_check_fails_on_a_lost_counter_carry():
    with pytest.raises(AssertionError, match="far offset") as e:
        sc.check_far_offsets_sens_philox(sc.StandIn("lost_carry"), 5)
    print(e.value)


@pytest.mark.parametrize("K", (4097, 8193))
def test_long_rows_check_fails_on_row_sums_that_stop_after_64_tiles(K):
    with pytest.raises(AssertionError, match="long rows") as e:
        sc.check_long_rows_sens_philox(sc.StandIn("mean_64_tiles"), 5, K)
    print(e.value)
    sc.check_long_rows_sens_philox(sc.StandIn("mean_64_tiles"), 5, 4096)


def test_long_rows_check_fails_on_a_mean_divided_by_the_tiles():
    with pytest.raises(AssertionError, match="long rows") as e:
        sc.check_long_rows_sens(sc.StandIn("mean_by_tiles"), 5, 4097)
    print(e.value)
