"""The checks of bootstrap_checks.py have teeth: every one passes on the stand-in (bootstrap.py, the definition) and every broken
variant of the stand-in fails at least one of them, the one named here included.  Runs without a GPU."""
import pytest

import bootstrap_checks as bc

# the check that has to see each defect (others may see it too)
CAUGHT_BY = {
    "zeros": bc.check_exact_permutation_rows,
    "same_indices_every_replicate": bc.check_exact_permutation_rows,
    "index_is_word_mod_K": bc.check_exact_permutation_rows,
    "words_reversed_in_quad": bc.check_two_valued_row,                  # (within a whole quad the order does not show: sums, min, counts)
    "counter_ignores_row": bc.check_rows_are_one_row_calls,
    "offset_ignored": bc.check_far_offsets,
    "std_ddof1_in_replicate": bc.check_exact_permutation_rows,
    "q_strictly_greater": bc.check_constant_row,
    "ranks_swapped": bc.check_summary_against_numpy,
}


@pytest.mark.parametrize("check", bc.ALL_CHECKS, ids=lambda c: c.__name__)
def test_stand_in_passes(check):
    if check is bc.check_ragged:
        check(bc.StandIn(), ks=(1, 3, 5, 65, 257), bs=(1, 5))          # (the device test runs the whole grid)
    else:
        check(bc.StandIn())


def test_every_defect_is_listed():
    assert set(CAUGHT_BY) == set(bc.BROKEN) and len(bc.BROKEN) == 9


@pytest.mark.parametrize("broken", bc.BROKEN)
def test_broken_variant_fails(broken):
    with pytest.raises(AssertionError):
        CAUGHT_BY[broken](bc.StandIn(broken))


def test_statistics_figures_of_the_definition():
    """the host definition on exactly the inputs of the device test: 188 of 200 rows covered, SE ratio in [0.913, 1.090]"""
    covered, lo, hi = bc.stat_figures(bc.StandIn())
    print(covered, lo, hi)
    assert covered == 188 and round(lo, 3) == 0.913 and round(hi, 3) == 1.090


def test_statistics_check_sees_a_wrong_stream():
    """identical indices in every replicate leave no spread at all: SE = 0, far outside [0.85, 1.15]"""
    with pytest.raises(AssertionError):
        bc.check_statistics(bc.StandIn("same_indices_every_replicate"))
