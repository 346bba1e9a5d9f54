"""Checks of a pairwise-Wasserstein backend against the definition (`wasserstein.matrix_reference`, math.fsum), shared by the CPU test
of the checks themselves (tests/test_wasserstein_checks.py: a NumPy stand-in passes, broken stand-ins fail) and the GPU tests
(tests/test_gpu_wasserstein.py).  A backend is any object with

    wasserstein_matrix(a, b=None, p=1, assume_sorted=False) -> ndarray (CA, CB)   (b=None: a against itself)

Each comparison is preceded by a teeth guard asserted on the REFERENCE alone: the data are such that the mistake the check is for
would move the answer by far more than the bar.  Bar: |err| <= (K + 4) 2^-52 W (`wasserstein.error_bar`: K - 1 additions of
non-negative terms in any order, the subtraction, the square, the division, the root)."""
import importlib

import numpy as np

wd = importlib.import_module("code-robchar_amd.wasserstein")

TILE = 64            # rcwd::kTile
CHUNK = 256          # rcwd::kChunk (the finest split of K)
RAGGED_C = (1, 2, 3, TILE - 1, TILE, TILE + 1, 2 * TILE + 3)
RAGGED_K = (1, 2, 7, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5)


class Standin:
    """The NumPy stand-in: the definition itself."""

    def wasserstein_matrix(self, a, b=None, p=1, assume_sorted=False):
        return wd.matrix_reference(a, b, p)


def beta_rows(C, K, seed, shape=(5.0, 1.5)):
    return np.random.default_rng(seed).beta(shape[0], shape[1], (C, K))


_REF = {}


def reference(key, a, b, p):
    """`matrix_reference`, computed once per named case and handed out read-only."""
    if key not in _REF:
        r = wd.matrix_reference(a, b, p)
        r.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def off_diagonal(W, symmetric):
    W = np.asarray(W)
    return W[~np.eye(W.shape[0], dtype=bool)] if symmetric else W.reshape(-1)


def assert_within_bar(got, want, K, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    err, bar = np.abs(got - want), wd.error_bar(want, K)
    ok = ~np.isnan(want)
    worst = float(np.max(np.where(ok, err / np.where(bar > 0, bar, 1.0), 0.0))) if ok.any() else 0.0
    print(f"{what}: shape {got.shape} K={K} worst error / bar = {worst:.3g}")
    assert np.all(err[ok] <= bar[ok]), (what, worst)


def check_general(be, CA=5, CB=3, K=300, seed=11):
    """Two different families, CA != CB, both p: division by K, the power, the orientation, and not all zeros."""
    a, b = np.sort(beta_rows(CA, K, seed), axis=1), np.sort(beta_rows(CB, K, seed + 1, (2.0, 2.0)), axis=1)
    w1, w2 = reference(("general", CA, CB, K, seed, 1), a, b, 1), reference(("general", CA, CB, K, seed, 2), a, b, 2)
    assert np.median(w1) >= 1e-2 and np.median(w2 - w1) >= 1e-3                  # teeth: zeros, and p ignored
    assert CA != CB                                                              # teeth: a transposed output has another shape
    for p, want in ((1, w1), (2, w2)):
        assert_within_bar(be.wasserstein_matrix(a, b, p=p, assume_sorted=True), want, K, f"general p={p}")


def check_sorting(be, C=6, K=257, seed=21):
    """Unsorted rows in, assume_sorted=False: the rows are sorted first."""
    a, b = beta_rows(C, K, seed), beta_rows(C, K, seed + 1, (2.0, 2.0))
    for p in (1, 2):
        want = reference(("sorting", C, K, seed, p), a, b, p)
        unsorted = np.abs(a[:, None, :] - b[None, :, :]).mean(-1) if p == 1 else np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).mean(-1))
        assert np.median(np.abs(want - unsorted)) >= 1e-2                         # teeth: rows not sorted
        assert_within_bar(be.wasserstein_matrix(a, b, p=p, assume_sorted=False), want, K, f"sorting p={p}")


def check_ragged_k(be, Ks=RAGGED_K, C=3, seed=31):
    """Every K around the step and chunk boundaries: the last partial chunk counts."""
    for K in Ks:
        a, b = np.sort(beta_rows(C, K, seed + K), axis=1), np.sort(beta_rows(C + 1, K, seed + K + 1, (2.0, 2.0)), axis=1)
        for p in (1, 2):
            want = reference(("ragged-k", C, K, seed, p), a, b, p)
            if K > CHUNK:                                                         # teeth: the values past the last whole chunk matter
                full = K // CHUNK * CHUNK
                cut = wd.matrix_reference(a[:, :full], b[:, :full], p)
                assert np.median(np.abs(cut - want) / wd.error_bar(want, K)) >= 1e3
            assert np.median(want) >= 1e-2 or K < 7
            assert_within_bar(be.wasserstein_matrix(a, b, p=p, assume_sorted=True), want, K, f"ragged K={K} p={p}")


def check_nan_rows(be, C=5, K=70, seed=41):
    """A NaN row gives NaN in exactly its row and column; every other element has the bits of the call without that row."""
    a, b = np.sort(beta_rows(C, K, seed), axis=1), np.sort(beta_rows(C + 2, K, seed + 1, (2.0, 2.0)), axis=1)
    an, bn = a.copy(), b.copy()
    an[1, K // 2] = np.nan
    bn[4] = np.nan
    for p in (1, 2):
        clean = np.asarray(be.wasserstein_matrix(a, b, p=p, assume_sorted=True))
        assert np.median(clean) >= 1e-2 and not np.isnan(clean).any()
        got = np.asarray(be.wasserstein_matrix(an, bn, p=p, assume_sorted=True))
        mask = np.zeros_like(clean, dtype=bool)
        mask[1, :] = True
        mask[:, 4] = True
        assert np.array_equal(np.isnan(got), mask), f"NaN pattern p={p}"
        assert np.array_equal(got[~mask], clean[~mask]), f"elements beside the NaN row p={p}"
        sym_clean = np.asarray(be.wasserstein_matrix(a, None, p=p, assume_sorted=True))
        sym = np.asarray(be.wasserstein_matrix(an, None, p=p, assume_sorted=True))
        smask = np.zeros_like(sym_clean, dtype=bool)
        smask[1, :] = True
        smask[:, 1] = True
        assert np.array_equal(np.isnan(sym), smask) and np.array_equal(sym[~smask], sym_clean[~smask]), f"symmetric NaN p={p}"


def check_symmetric(be, C=TILE + 6, K=40, seed=51):
    """b=None: the matrix of a against itself - equal to the general call on a copy, to its transpose, zero diagonal - over more
    than one tile, so that a mirror image written to the wrong place shows."""
    a = np.sort(beta_rows(C, K, seed) * np.linspace(0.3, 1.0, C)[:, None], axis=1)
    for p in (1, 2):
        want = reference(("symmetric", C, K, seed, p), a, None, p)
        assert np.median(off_diagonal(want, True)) >= 1e-2
        assert np.median(np.abs(want - np.roll(want, 1, axis=0))) >= 1e-3            # teeth: rows of the matrix differ from their neighbours
        got = np.asarray(be.wasserstein_matrix(a, None, p=p, assume_sorted=True))
        assert_within_bar(got, want, K, f"symmetric p={p}")
        assert np.array_equal(got, got.T) and np.all(np.diag(got) == 0.0)
        assert np.array_equal(got, np.asarray(be.wasserstein_matrix(a, a.copy(), p=p, assume_sorted=True)))


ALL = (check_general, check_sorting, check_ragged_k, check_nan_rows, check_symmetric)


# ---- exact known answers on a dyadic grid: every sum is exact in any order ------------------------------------------------------
GRID = 20            # values are integers in [0, 2^GRID] times 2^-GRID


def grid_rows(C, K, seed):
    """(C, K) sorted int64 rows, row r uniform in [0, 2^20 (r + 1) / C] (rows of different spread: their distances are of order
    0.1); K <= 4096 keeps sum d^2 below 2^52 grid units."""
    assert K <= 4096
    hi = (2 ** GRID * (np.arange(C) + 1)) // C
    return np.sort(np.random.default_rng(seed).integers(0, hi[:, None] + 1, (C, K)), axis=1)


def grid_values(rows):
    return rows.astype(np.float64) * 2.0 ** -GRID


def grid_answer(ra, rb, p):
    """The exact answer from integer arithmetic: the integer sum, scaled (exactly), divided ONCE by K, and np.sqrt for p = 2."""
    K = ra.shape[1]
    d = ra[:, None, :].astype(object) - rb[None, :, :].astype(object)
    s = np.abs(d).sum(-1) if p == 1 else (d * d).sum(-1)
    scale = 2.0 ** (-GRID * p)
    mean = np.array([[float(int(v)) * scale / K for v in row] for row in s])         # (int -> float exact: below 2^53)
    assert all(int(v) < 2 ** 53 for row in s for v in row)
    return mean if p == 1 else np.sqrt(mean)
