"""The checks of tests/variance_checks.py pass on the NumPy stand-in (oracle `fidelity_eigh` on `philox_host` draws + the definition
module) and FAIL on every deliberately broken stand-in - so the GPU tests that run the same checks on the device can fail too."""
import pytest

import variance_checks as vc


@pytest.mark.parametrize("N,K,pair", ((3, 65, (0, 2)), (4, 63, (1, 2))))
def test_checks_pass_on_the_stand_in(N, K, pair):
    vc.run_all(vc.StandIn(), N, K, pair)


@pytest.mark.parametrize("broken", vc.BROKEN)
def test_checks_fail_on_a_broken_stand_in(broken):
    with pytest.raises(AssertionError):
        vc.run_all(vc.StandIn(broken), 3, 65, (0, 2))
    # ... and each mistake is caught by the check that is about it
    check = vc.check_means_against_own_slabs if broken in ("t_u_exchanged", "mean_over_tiles") else vc.check_against_reference
    with pytest.raises(AssertionError):
        check(vc.StandIn(broken), 3, 65, 0, 2)
