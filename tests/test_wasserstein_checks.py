"""The checks of tests/wasserstein_checks.py have teeth: the NumPy stand-in built on `wasserstein.matrix_reference` passes every one
of them, and each broken stand-in - a mistake the device code could make - fails at least one.  Runs without a GPU."""
import numpy as np
import pytest

import wasserstein_checks as wc

wd = wc.wd


def _sorted(a, b, assume_sorted):
    if assume_sorted:
        return a, (a if b is None else b)
    return np.sort(a, axis=1), np.sort(a if b is None else b, axis=1)


def _power_mean(d, p, K):
    return np.abs(d).sum(-1) / K if p == 1 else np.sqrt((d * d).sum(-1) / K)


class Broken(wc.Standin):
    """A plain NumPy implementation (not the definition: pairwise-summed, inside the bar) with one switchable mistake."""

    def __init__(self, mistake):
        self.mistake = mistake

    def wasserstein_matrix(self, a, b=None, p=1, assume_sorted=False):
        m = self.mistake
        a = np.asarray(a, dtype=np.float64)
        sa, sb = _sorted(a, None if b is None else np.asarray(b, dtype=np.float64), assume_sorted or m == "unsorted")
        K = a.shape[1]
        if m == "chunk":
            full = K // wc.CHUNK * wc.CHUNK if K > wc.CHUNK else K
            sa, sb = sa[:, :full], sb[:, :full]
        d = sa[:, None, :] - sb[None, :, :]
        if m == "nan":
            d = np.nan_to_num(d, nan=0.0)
        out = _power_mean(d, 1 if m == "p" else p, 1 if m == "nodiv" else K)
        if m == "transposed":
            out = np.ascontiguousarray(out.T)
        if m == "mirror" and b is None:                  # the tiles below the diagonal come from the wrong tile
            out = np.triu(out)
            T = wc.TILE
            for i in range(T, out.shape[0]):
                out[i, :T] = out[:T, i][::-1]
            out = np.where(np.tri(out.shape[0], k=-1, dtype=bool) & (out == 0), out.T, out)
        if m == "zeros":
            out = np.zeros_like(out)
        return out


MISTAKES = ("unsorted", "nodiv", "p", "transposed", "chunk", "nan", "mirror", "zeros")


@pytest.mark.parametrize("check", wc.ALL, ids=lambda f: f.__name__)
def test_the_definition_passes(check):
    check(wc.Standin())


@pytest.mark.parametrize("check", wc.ALL, ids=lambda f: f.__name__)
def test_a_correct_plain_implementation_passes(check):
    check(Broken(None))


@pytest.mark.parametrize("mistake", MISTAKES)
def test_every_mistake_is_caught(mistake):
    failed = []
    for check in wc.ALL:
        try:
            check(Broken(mistake))
        except AssertionError:
            failed.append(check.__name__)
    print(mistake, "caught by", failed)
    assert failed, mistake


def test_reference_properties():
    """the definition: symmetric, zero diagonal, W_1 <= W_2, RIM against a row of ones, NaN propagation, sorts its input"""
    a = wc.beta_rows(4, 50, 3)
    for p in (1, 2):
        w = wd.matrix_reference(a, None, p)
        assert np.array_equal(w, w.T) and np.all(np.diag(w) == 0)
        assert np.array_equal(w, wd.matrix_reference(np.sort(a, axis=1)[:, ::-1], a, p))
    assert np.all(wd.matrix_reference(a, None, 1) <= wd.matrix_reference(a, None, 2) + 1e-15)
    ones = np.ones((1, 50))
    assert np.allclose(wd.matrix_reference(a, ones, 1)[:, 0], 1.0 - a.mean(1), rtol=0, atol=1e-15)
    assert np.allclose(wd.matrix_reference(a, ones, 2)[:, 0], np.sqrt(((1.0 - a) ** 2).mean(1)), rtol=0, atol=1e-15)
    a[2, 7] = np.nan
    w = wd.matrix_reference(a, None, 1)
    assert np.isnan(w[2]).all() and np.isnan(w[:, 2]).all() and np.isnan(w).sum() == 7
    with pytest.raises(ValueError):
        wd.matrix_reference(a, None, 3)
    with pytest.raises(ValueError):
        wd.matrix_reference(a, np.ones((2, 49)), 1)


def test_grid_answers_are_the_definition():
    """the integer-arithmetic answers of the exact tests equal the fsum reference to its rounding"""
    ra, rb = wc.grid_rows(3, 100, 5), wc.grid_rows(2, 100, 6)
    for p in (1, 2):
        exact, ref = wc.grid_answer(ra, rb, p), wd.matrix_reference(wc.grid_values(ra), wc.grid_values(rb), p)
        assert np.median(exact) >= 1e-2 and np.all(np.abs(exact - ref) <= 2.0 ** -51 * exact)
    assert np.array_equal(wc.grid_answer(ra, ra, 1).diagonal(), np.zeros(3))
