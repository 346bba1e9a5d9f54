"""The checks of listed_checks.py on a NumPy stand-in: every check passes on the right one, and each broken stand-in - weights
ignored, an empty slot counted, the list index taken as the slot number, the row offset c K dropped, the row sum stopping after
64 tiles - fails the check that is there to catch it.  CPU only."""
import numpy as np
import pytest

import listed_checks as lc

GOOD = lc.StandIn()


def test_every_check_passes_on_the_stand_in():
    lc.check_reference(GOOD, 7, lengths=(1, 65))
    lc.check_identity(GOOD, 7)
    lc.check_position_independence(GOOD, 7)
    lc.check_weights(GOOD, 7)
    lc.check_long_rows(GOOD, 4097)
    lc.check_modes(GOOD, 7)
    lc.check_hard_inputs(GOOD, 7)


@pytest.mark.parametrize("broken, check", [
    ("weights_ignored", lambda be: lc.check_weights(be, 7)),
    ("weights_ignored", lambda be: lc.check_reference(be, 7, lengths=(65,))),
    ("empty_counted", lambda be: lc.check_reference(be, 7, lengths=(65,))),
    ("empty_counted", lambda be: lc.check_weights(be, 7)),
    ("index_as_slot", lambda be: lc.check_reference(be, 7, lengths=(65,))),
    ("index_as_slot", lambda be: lc.check_position_independence(be, 7)),
    ("row_offset_dropped", lambda be: lc.check_reference(be, 7, lengths=(65,))),
    ("row_offset_dropped", lambda be: lc.check_modes(be, 7)),
    ("sum_64_tiles", lambda be: lc.check_long_rows(be, 4097)),
])
def test_a_broken_stand_in_fails_its_check(broken, check):
    with pytest.raises(AssertionError):
        check(lc.StandIn(broken))


def test_the_broken_sum_passes_up_to_64_tiles():
    """(so it is the 65th tile that check_long_rows(4097) catches, not something else)"""
    lc.check_long_rows(lc.StandIn("sum_64_tiles"), 4096)


def test_tail_reference_by_hand():
    F = np.array([[0.5, 0.1, 0.9, 0.3, 0.7]])
    listed, weights, gap = lc.tail_reference(F, 0.5)                  # alpha K = 2.5: the 3 smallest, the third with weight 0.5 / 2.5
    assert listed.tolist() == [[0, 1, 3]]
    assert np.allclose(weights, [[0.2, 0.4, 0.4]]) and abs(gap[0] - 0.2) < 1e-15
    G = np.arange(10.0).reshape(1, 5, 2)
    cvar, grad, var, _ = lc.cvar_reference(F, G, 0.5)
    assert abs(cvar[0] - (0.4 * 0.1 + 0.4 * 0.3 + 0.2 * 0.5)) < 1e-15 and var[0] == 0.5
    assert np.allclose(grad[0], 0.4 * G[0, 1] + 0.4 * G[0, 3] + 0.2 * G[0, 0])
