"""The checks of tests/times_checks.py pass on the NumPy stand-in built on `orc.fidelity_eigh` and fail on each deliberately
broken one - runs without a GPU.  What tests/test_gpu_times.py asserts on the device is asserted here on the oracle first."""
import numpy as np
import pytest

import times_checks as tc


@pytest.fixture(scope="module")
def good():
    return tc.StandIn()


@pytest.mark.parametrize("N,a,b", tc.PAIRS)
def test_oracle_workloads_have_teeth_and_pass(good, N, a, b):
    """the reference satisfies both guards with room on every pair of the GPU comparison"""
    _, _, want = tc.oracle_workload(N, a, b)
    spread = tc.check_reference_guards(want, (N, a, b))
    med, share = float(np.median(want)), float((want > 1e-3).mean())
    print(f"N={N} ({a},{b}): median F {med:.3f}, share > 1e-3 {share:.3f}, median spread {spread:.3f}")
    assert 0.04 <= med <= 0.75 and share >= 0.98 and 0.09 <= spread <= 0.61
    tc.check_oracle(good, N, a, b)
    assert tc.check_against_rows_kernel(good, N, a, b) == 0.0


@pytest.mark.parametrize("N,a,b", [p for p in tc.EVERY_SIZE if p not in tc.PAIRS])
def test_every_size_has_teeth_and_passes(good, N, a, b):
    """the sizes and pairs the GPU comparison adds to PAIRS: both guards hold on the reference (the margins are smaller than on
    PAIRS: the worst median F is 0.034 and the worst spread 0.084, both at N = 15, 7 -> 6; the smallest share above 1e-3 is 0.981)"""
    _, _, want = tc.oracle_workload(N, a, b)
    spread = tc.check_reference_guards(want, (N, a, b))
    print(f"N={N} ({a},{b}): median F {float(np.median(want)):.3f}, share > 1e-3 {float((want > 1e-3).mean()):.3f}, median spread {spread:.3f}")
    tc.check_oracle(good, N, a, b)
    assert tc.check_against_rows_kernel(good, N, a, b) == 0.0


def test_every_size_is_listed():
    assert {p[0] for p in tc.EVERY_SIZE} == set(range(2, 17)) and set(tc.PAIRS) <= set(tc.EVERY_SIZE) and len(tc.EVERY_SIZE) == 34
    assert (2, 1, 0) in tc.EVERY_SIZE and (15, 7, 6) in tc.EVERY_SIZE


@pytest.mark.parametrize("N", sorted(set(tc.STEP_SIZES) | {3, 7, 16}))
def test_closed_form(good, N):
    tc.check_closed_form(good, N)


def test_semantics_and_edges(good):
    tc.check_semantics(good)
    tc.check_edges(good)


@pytest.mark.parametrize("broken", tc.StandIn.BROKEN)
def test_broken_stand_ins_fail(broken):
    with pytest.raises(AssertionError):
        tc.check_semantics(tc.StandIn(broken))


@pytest.mark.parametrize("broken", ("ignores tscale", "ignores tshift", "slabs reversed", "slab layout [C][K][M]"))
def test_broken_grids_fail_the_oracle_comparison(broken):
    """the comparison the GPU suite runs on every (N, in, out) catches a wrong grid on its own"""
    with pytest.raises(AssertionError):
        tc.check_oracle(tc.StandIn(broken), 7, 0, 6)


def test_weighted_sum_is_the_fma_sequence():
    """the exact fma of the checks against a case where fma and multiply-then-add differ"""
    a, b, c = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30, -1.0
    assert tc._fma(a, b, c) == -(2.0 ** -60) and a * b + c == 0.0
    w = np.array([0.5, a])
    slabs = np.array([[-2.0], [b]])
    assert tc.weighted_sum(w, slabs)[0] == -(2.0 ** -60)
    assert np.isnan(tc.weighted_sum(w, np.array([[np.nan], [1.0]]))[0])
