"""The checks of tests/variance_checks.py pass on the NumPy stand-in (oracle `fidelity_eigh` on `philox_host` draws + the definition
module) and FAIL on every deliberately broken stand-in - so the GPU tests that run the same checks on the device can fail too."""
import pytest

import variance_checks as vc


@pytest.mark.parametrize("N,K,pair", ((3, 65, (0, 2)), (4, 63, (1, 2))))
def test_checks_pass_on_the_stand_in(N, K, pair):
    vc.run_all(vc.StandIn(), N, K, pair)


@pytest.mark.parametrize("broken", [b for b in vc.BROKEN if b not in vc.LONG_ROW_BROKEN])
def test_checks_fail_on_a_broken_stand_in(broken):
    with pytest.raises(AssertionError):
        vc.run_all(vc.StandIn(broken), 3, 65, (0, 2))
    # ... and each mistake is caught by the check that is about it
    check = vc.check_means_against_own_slabs if broken in ("t_u_exchanged", "mean_over_tiles") else vc.check_against_reference
    with pytest.raises(AssertionError):
        check(vc.StandIn(broken), 3, 65, 0, 2)


def test_long_rows_pass_on_the_stand_in_and_fail_when_the_tiles_behind_the_64th_are_dropped():
    """K = 4097 is 65 tiles: the 65th is the second step of lane 0 in the row-mean kernel.  The broken stand-in is right at every K
    the other checks use (`run_all` passes on it), so only the long-row check can see it."""
    vc.check_long_rows(vc.StandIn(), 2, 4097)
    with pytest.raises(AssertionError, match="row means"):
        vc.check_long_rows(vc.StandIn("mean_first_64_tiles"), 2, 4097)
    vc.run_all(vc.StandIn("mean_first_64_tiles"), 3, 65, (0, 2))
    vc.check_long_rows(vc.StandIn("mean_first_64_tiles"), 2, 4096)      # one tile per lane: nothing is dropped yet


def test_group_count_edges_on_the_stand_in():
    """G = 0 and G = 64 (every subset of the 6 coordinates at N = 2) on the stand-in; a stand-in that writes the group slabs one
    place off fails the exhaustive check"""
    vc.check_no_groups(vc.StandIn(), 3)
    vc.check_every_subset(vc.StandIn(), 65)
    with pytest.raises(AssertionError):
        vc.check_every_subset(vc.StandIn("slab_one_off"), 65)
    with pytest.raises(AssertionError):
        vc.check_every_subset(vc.StandIn("index_3s_plus_i"), 65)
    masks = vc.limit_masks()
    assert len(masks) == 64 and len(set(masks.tolist())) == 64 and (masks[39:] >> vc.np.uint64(32) != 0).all() and int(masks.max()) < 2 ** 39
