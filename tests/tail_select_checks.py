"""Data-level checks of a tail selection `select(fid (C, K) float64 NumPy array, alpha) -> (list (C, m) int32, weight (C, m), var (C,))`
(NumPy arrays): `backend.tail_select` on the device, the NumPy route of `noise.tail_weights`, the serial select of
tests/host/host_tail_select.cpp - and the broken stand-ins of tests/test_tail_select_checks.py, each of which one of the checks
must catch.  Every comparison is exact (np.array_equal); there is no tolerance anywhere.

The reference is `listed_checks.tail_reference` - a sort by (value, index) written independently of `tail_weights` - with the value
at risk from np.sort; a row with a NaN is expected as list = -1, weight = 0.0, var = NaN.  A case's inputs and reference are
computed once per process and shared (read-only) by every select that is checked."""
import math

import numpy as np

import listed_checks as lc

RANDOM_K = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097, 10_000, 16_384, 16_385, 100_003)
TIE_CASES = ((1000, 0.1), (10_000, 0.03), (16_385, 0.1), (100_003, 0.01))
CONSTANT_M = (1, 63, 64, 65, 255, 256, 257, 512, 1023, 1024)
SPECIAL_ALPHAS = (0.5 / 257, 0.2, 0.28, 0.5, 1.0)

_CASES = {}


def tail_len(K, alpha):
    return min(K, int(math.ceil(alpha * K)))


def random_alphas(K):
    """m = 1, three fractions, m = K with a fractional last weight (wherever 0.95 K > K - 1), and the mean"""
    return (0.5 / K, 0.03, 0.1, 0.5, 0.95, 1.0)


def expected(F, alpha):
    C, K = F.shape
    m = tail_len(K, alpha)
    ok = ~np.isnan(F).any(axis=1)
    lst, w, var = np.full((C, m), -1, dtype=np.int32), np.zeros((C, m)), np.full(C, np.nan)
    if ok.any():
        lst[ok], w[ok], _ = lc.tail_reference(F[ok], alpha)
        var[ok] = np.sort(F[ok], axis=1)[:, m - 1]
    return lst, w, var


def case(tag, make, alpha):
    """(F, (list, weight, var)) of a named case, computed once; `make` -> F"""
    key = (tag, alpha)
    if key not in _CASES:
        fkey = (tag, None)
        if fkey not in _CASES:
            F = np.ascontiguousarray(make(), dtype=np.float64)
            F.setflags(write=False)
            _CASES[fkey] = F
        F = _CASES[fkey]
        exp = expected(F, alpha)
        for a in exp:
            a.setflags(write=False)
        _CASES[key] = (F, exp)
    return _CASES[key]


def compare(select, F, exp, tag):
    got = select(F.copy(), tag[-1])
    assert len(got) == 3, tag
    for name, g, e in zip(("list", "weight", "var"), got, exp):
        g = np.asarray(g)
        assert g.shape == e.shape, (tag, name, g.shape, e.shape)
        assert g.dtype == e.dtype, (tag, name, g.dtype)
        assert np.array_equal(g, e, equal_nan=(name == "var")), (tag, name)
    return got


# ------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------


def random_rows(K, C=5):
    def make():
        F = np.random.default_rng(4000 + K + 17 * C).random((C, K))
        if C >= 3:
            F[2, K // 2] = np.nan
        return F
    return make


def tie_rows(K):
    return lambda: np.floor(16.0 * np.random.default_rng(1234 + K).random((5, K))) / 16.0


def last_digit_rows():
    j = np.random.default_rng(7).permutation(1000)
    return (0.5 + j * 2.0 ** -53)[None, :]


def special_rows():
    """K = 257: -inf, +inf, 40 values in (-1, 0), 30 zeros (+0.0 and -0.0, 15 of each), 5 denormals 5e-324, the rest in (1, 2): two
    rows in random index order, one in the order just named"""
    rng = np.random.default_rng(257)
    zeros = np.where(np.arange(30) % 2 == 0, 0.0, -0.0)
    vals = np.concatenate([[-np.inf, np.inf], -rng.uniform(1e-3, 1.0, 40), zeros, np.full(5, 5e-324),
                           1.0 + rng.uniform(1e-3, 1.0, 257 - 77)])
    rows = np.stack([vals[rng.permutation(257)], vals[rng.permutation(257)][::-1], vals])
    return rows


def key_bits(F):
    """the order-preserving unsigned keys of csrc/select_core.h, in NumPy"""
    F = np.where(F == 0.0, 0.0, F)
    u = np.ascontiguousarray(F, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))


# ------------------------------------------------------------------------------------------------------------------------
# checks
# ------------------------------------------------------------------------------------------------------------------------


def check_random(select, ks=RANDOM_K, which=range(6)):
    """`which`: indices into random_alphas(K) (the tests take one (K, alpha) pair per case)"""
    for K in ks:
        for alpha in (random_alphas(K)[j] for j in which):
            F, exp = case(("random", K), random_rows(K), alpha)
            compare(select, F, exp, ("random", K, alpha))
            if K > 1 and alpha == 0.95 and 0.95 * K > K - 1:
                assert exp[0].shape[1] == K and exp[1][0].min() < 1.0 / (0.95 * K)      # m = K with a fractional last weight


def check_one_row_and_paper_rows(select):
    F, exp = case(("one row", 1000), random_rows(1000, C=1), 0.1)
    compare(select, F, exp, ("one row", 1000, 0.1))
    F, exp = case(("paper rows", 100), random_rows(100, C=2048), 0.1)
    compare(select, F, exp, ("paper rows", 100, 0.1))


def check_ties(select, cases=TIE_CASES):
    for K, alpha in cases:
        F, exp = case(("ties", K), tie_rows(K), alpha)
        thr = exp[2][:, None]
        total = (F == thr).sum(axis=1)
        chosen = (np.take_along_axis(F, exp[0].astype(np.int64), 1) == thr).sum(axis=1)
        assert (total > chosen).all() and (chosen >= 1).all(), (K, alpha, total, chosen)       # the threshold splits a tie group
        compare(select, F, exp, ("ties", K, alpha))


def check_constant_rows(select, ms=CONSTANT_M):
    for m in ms:
        alpha = m / 1024.0
        F, exp = case(("constant", 1024), lambda: np.full((2, 1024), 0.75), alpha)
        assert np.array_equal(exp[0], np.tile(np.arange(m, dtype=np.int32), (2, 1)))
        assert (exp[1][:, :m - 1] == 1.0 / m).all() and (exp[1][:, m - 1] == (m - (m - 1)) / float(m)).all()
        compare(select, F, exp, ("constant", 1024, alpha))


def check_last_digit(select):
    F, exp = case(("last digit", 1000), last_digit_rows, 0.1)
    keys = key_bits(F[0])
    assert len(set((keys >> np.uint64(16)).tolist())) == 1 and len(set(keys.tolist())) == 1000
    compare(select, F, exp, ("last digit", 1000, 0.1))


def check_special_values(select, alphas=SPECIAL_ALPHAS):
    for alpha in alphas:
        F, exp = case(("special", 257), special_rows, alpha)
        if alpha == 0.2:          # the threshold is zero and splits the zeros: both signs are selected, and some of each are not
            sel = np.take_along_axis(F, exp[0].astype(np.int64), 1)
            for row, s in zip(F, sel):
                z = s[s == 0.0]
                assert 0 < z.size < 30 and np.signbit(z).any() and not np.signbit(z).all()
            assert (exp[2] == 0.0).all()
        if alpha == 0.28:         # ... and here the denormals
            assert (exp[2] == 5e-324).all()
        compare(select, F, exp, ("special", 257, alpha))


def check_repeat(select):
    """a second call gives the same bits"""
    F, exp = case(("ties", 1000), tie_rows(1000), 0.1)
    a = compare(select, F, exp, ("ties", 1000, 0.1))
    b = compare(select, F, exp, ("ties", 1000, 0.1))
    for x, y in zip(a, b):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


ALL_CHECKS = (check_random, check_one_row_and_paper_rows, check_ties, check_constant_rows, check_last_digit, check_special_values,
              check_repeat)
