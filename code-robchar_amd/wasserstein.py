"""The definition, in NumPy, of the pairwise Wasserstein matrix that `rc_wasserstein_matrix_f64` computes on the GPU
(include/robchar_hip.h, ABI 18; kernels: csrc/k_wasserstein.inc.h).

For two samples a, b of equal size K the p-Wasserstein distance between their empirical distributions is the l_p distance of the
sorted samples,

    W_1 = (1/K) sum_k |a_(k) - b_(k)|,        W_2 = sqrt((1/K) sum_k (a_(k) - b_(k))^2),

and a row of ones as b gives RIM_p, the distance to the ideal distribution delta(F - 1) that `rim_metrics` reports.  The reference
here sums with `math.fsum` (exactly rounded), so it carries no summation error of its own: the device result may differ from it by
its own rounding only, at most (K + 4) 2^-52 W (K - 1 additions of non-negative terms, the subtraction, the square, the division
and the root).  The checks (tests/wasserstein_checks.py) and the CPU stand-in of the tests are built on it; the product never calls
it on the hot path.
"""
from __future__ import annotations

import math

import numpy as np


def pair_reference(a_sorted, b_sorted, p: int = 1) -> float:
    """W_p of two SORTED rows of equal length (NaN if either holds one)."""
    d = np.asarray(a_sorted, dtype=np.float64) - np.asarray(b_sorted, dtype=np.float64)
    if np.isnan(d).any():
        return float("nan")
    if p == 1:
        return math.fsum(np.abs(d).tolist()) / d.size
    return math.sqrt(math.fsum((d * d).tolist()) / d.size)


def matrix_reference(a, b=None, p: int = 1) -> np.ndarray:
    """out[i, j] = W_p(a[i], b[j]) for the rows of a (CA, K) and b (CB, K) - sorted here; `b=None`: a against itself.  A row holding
    a NaN gives NaN in its whole row and column."""
    if p not in (1, 2):
        raise ValueError("p must be 1 or 2")
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2 or (b is not None and (np.ndim(b) != 2 or np.shape(b)[1] != a.shape[1])):
        raise ValueError("a: expected (CA, K), b: (CB, K) with the same K")
    sa = np.sort(a, axis=1)                                    # (NaN sorts last: the row still holds it)
    sb = sa if b is None else np.sort(np.asarray(b, dtype=np.float64), axis=1)
    K = a.shape[1]
    out = np.empty((sa.shape[0], sb.shape[0]))
    for i in range(sa.shape[0]):
        j0 = i if b is None else 0                             # a against itself: the upper triangle, mirrored
        d = sa[i][None, :] - sb[j0:]
        terms = np.abs(d) if p == 1 else d * d                 # (d * d is rounded once per term, which the device's fma is not:
        sums = np.array([math.fsum(r) for r in terms.tolist()]) if K else np.zeros(d.shape[0])   # 1 ulp of a term, inside the bar)
        sums[np.isnan(terms).any(axis=1)] = np.nan             # (fsum of a NaN is a NaN already; spelled out)
        with np.errstate(invalid="ignore", divide="ignore"):
            out[i, j0:] = sums / K if p == 1 else np.sqrt(sums / K)
        if b is None:
            out[j0:, i] = out[i, j0:]
    return out


def error_bar(W, K: int):
    """The bound on |device - matrix_reference|: (K + 4) 2^-52 W."""
    return (K + 4) * 2.0 ** -52 * np.asarray(W)
