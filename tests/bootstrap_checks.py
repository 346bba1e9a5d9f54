"""Checks of the bootstrap of the metrics (`backend.bootstrap_metrics`, rc_bootstrap_metrics_f64*): references built on
`oracle/philox_host.philox4x32_10`, independent of the package's own restatement; a `StandIn` backend built on
`code-robchar_amd/bootstrap.py`; broken variants of it.  Every `check_*` takes a backend - an object with `bootstrap_metrics` that
takes NumPy arrays and returns NumPy arrays - and is run on the stand-in and its broken variants on the CPU
(test_bootstrap_checks.py) and on the device (test_gpu_bootstrap.py).

Tolerances.  Values lie in [0, 1].  A sum of K such values in any order carries an error of at most gamma_K max|sum| < K^2 2^-53,
i.e. K 2^-53 on the mean; the bounds used are twice that: |mean - fsum mean| <= K 2^-52.  The variance is a mean of squares of
g = f - m in [-1, 1] (error K 2^-53 and the rounding of g, 2^-53 each, times 2|g|) minus a squared mean: 4 K 2^-52 covers it.
No tolerance here comes from a measured figure."""
import importlib
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import philox_host  # noqa: E402

boot = importlib.import_module("code-robchar_amd.bootstrap")

Q = (0.95, 0.98)
U = 2.0 ** -52
RAGGED_K = (1, 3, 4, 5, 63, 64, 65, 257, 1000)
RAGGED_B = (1, 2, 5, 67)
ERRORS = (ValueError, RuntimeError)


# ---- references on the oracle's Philox ---------------------------------------------------------------------------------------------
def ref_indices(K, B, seed, offset, c=0):
    """(B, K) indices of row c: word t & 3 of counter offset + (c B + b) Q + (t >> 2), idx = (word K) >> 32"""
    Qd = (K + 3) // 4
    out = np.empty((B, K), dtype=np.int64)
    t = np.arange(K)
    for b in range(B):
        ctr = [(offset + (c * B + b) * Qd + q) % 2 ** 64 for q in range(Qd)]
        lo = np.array([v & 0xFFFFFFFF for v in ctr], dtype=np.uint64)
        hi = np.array([v >> 32 for v in ctr], dtype=np.uint64)
        w = np.stack(philox_host.philox4x32_10(lo, hi, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))     # (4, Q)
        word = w[t & 3, t >> 2].astype(np.uint64)
        out[b] = ((word * np.uint64(K)) >> np.uint64(32)).astype(np.int64)
    return out


def ref_gathered(F, B, seed, offset):
    """list over rows of the (B, K) gathered values (None for a NaN row)"""
    C, K = F.shape
    return [None if np.isnan(F[c]).any() else F[c][ref_indices(K, B, seed, offset, c)] for c in range(C)]


def ref_exact_replicates(F, B, seed, offset, thr):
    """Replicates in the definition's formulas with plain float64 sums: exact whenever every sum is (see exact_rows)."""
    C, K = F.shape
    out = np.full((3 + len(thr), C, B), np.nan)
    for c, f in enumerate(ref_gathered(F, B, seed, offset)):
        if f is None:
            continue
        m = F[c].sum() / K
        g = f - m
        mg = g.sum(axis=1) / K
        out[0, c] = 1.0 - (m + mg)
        out[1, c] = (g * g).sum(axis=1) / K - mg * mg                   # the VARIANCE: the root is compared through its square
        out[2, c] = f.min(axis=1)
        for i, t in enumerate(thr):
            out[3 + i, c] = (f >= t).sum(axis=1) / K
    return out


def exact_rows(C=3, K=256, seed=5):
    """rows that are permutations of k / 256: with m = 255 / 512 every g is a multiple of 2^-9 below 1, every g^2 a multiple of
    2^-18: all sums of K = 256 of them are exact in float64 in any order, and so are S1 / K, its square and S2 / K"""
    rng = np.random.default_rng(seed)
    F = np.stack([rng.permutation(K) / 256.0 for _ in range(C)])
    assert K == 256
    g = F - F.sum(axis=1, keepdims=True) / K
    assert np.all(g * 512.0 == np.round(g * 512.0)) and np.all((g * g) * 2.0 ** 18 == np.round((g * g) * 2.0 ** 18))
    return F


def _call(be, F, B, seed, **kw):
    kw.setdefault("q_thresholds", Q)
    return be.bootstrap_metrics(np.ascontiguousarray(F), B, seed, **kw)


def assert_exact_against_host(be, F, B, seed, offset, thr=(0.25, 0.5, 0.95), **kw):
    res = _call(be, F, B, seed, offset=offset, q_thresholds=thr, **kw)
    rep, want = res["replicates"], ref_exact_replicates(F, B, seed, offset, thr)
    assert rep.shape == want.shape == (3 + len(thr), F.shape[0], B)
    for j in (0, 2, 3, 4, 5)[:2 + len(thr)]:
        assert rep[j].tobytes() == want[j].tobytes(), (res["names"][j], offset, np.argwhere(rep[j] != want[j])[:4])
    var = want[1]
    assert np.all(np.abs(rep[1] ** 2 - var) <= 2.0 * np.spacing(var)), np.abs(rep[1] ** 2 - var).max()
    return res


# ---- 1. exact known answers from the indices alone -------------------------------------------------------------------------------
def check_exact_permutation_rows(be):
    res = assert_exact_against_host(be, exact_rows(), 33, 0x5EED0001, 0)
    assert tuple(res["names"]) == ("rim1", "std", "min", "q0", "q1", "q2")
    assert len(np.unique(res["replicates"][0])) > 60                 # the replicates differ from each other and between rows


def check_constant_row(be):
    F = np.full((2, 100), 0.75)
    res = _call(be, F, 20, 3, q_thresholds=(0.75, 0.76))
    rep, s = res["replicates"], res["summary"]
    assert np.all(rep[0] == 0.25) and np.all(rep[1] == 0.0) and np.all(rep[2] == 0.75) and np.all(rep[3] == 1.0) and np.all(rep[4] == 0.0)
    assert np.all(s[:, 1] == 0.0) and np.all(s[:, 2] == s[:, 3])
    assert np.all(s[0, 0] == 0.25) and np.all(s[0, 2] == 0.25) and np.all(s[3, 0] == 1.0)


def check_two_valued_row(be):
    K, B, seed, offset = 301, 40, 9, 11                  # (no multiple of four: the last quad is cut, so the word order shows)
    F = np.where(np.arange(2 * K).reshape(2, K) % 3 == 0, 0.99, 0.5)
    rep = _call(be, F, B, seed, offset=offset, q_thresholds=(0.99, 0.5, 0.995))["replicates"]
    for c, f in enumerate(ref_gathered(F, B, seed, offset)):
        count = (f == 0.99).sum(axis=1)
        assert np.array_equal(rep[3, c], count / K) and np.all(rep[4, c] == 1.0) and np.all(rep[5, c] == 0.0)
        assert np.array_equal(rep[2, c], np.where(count < K, 0.5, 0.99))
        assert 0 < count.min() and count.max() < K and len(np.unique(count)) > 5


# ---- 2. ragged shapes ----------------------------------------------------------------------------------------------------------------
def ragged_fid(K):
    F = np.random.default_rng(1000 + K).random((3, K))
    F[1, K // 2] = np.nan
    return F


def check_ragged(be, ks=RAGGED_K, bs=RAGGED_B):
    for K in ks:
        F = ragged_fid(K)
        for B in bs:
            res = _call(be, F, B, 21, offset=7)
            rep, s = res["replicates"], res["summary"]
            assert rep.shape == (5, 3, B) and s.shape == (5, 4, 3)
            assert np.isnan(rep[:, 1]).all() and np.isnan(s[:, :, 1]).all()
            assert np.isfinite(rep[:, (0, 2)]).all() and np.isfinite(s[:, (0, 2, 3)][:, :, (0, 2)]).all()
            assert np.isnan(s[:, 1]).all() if B == 1 else np.isfinite(s[:, 1][:, (0, 2)]).all()
            for c, f in enumerate(ref_gathered(F, B, 21, 7)):
                if f is None:
                    continue
                for b in range(B):
                    mean = math.fsum(f[b]) / K
                    var = math.fsum((f[b] - mean) ** 2) / K
                    assert rep[2, c, b] == f[b].min(), (K, B, c, b)
                    assert rep[3, c, b] == (f[b] >= Q[0]).sum() / K and rep[4, c, b] == (f[b] >= Q[1]).sum() / K, (K, B, c, b)     # q K = the count
                    assert abs((1.0 - rep[0, c, b]) - mean) <= K * U, (K, B, c, b, (1.0 - rep[0, c, b]) - mean)
                    assert abs(rep[1, c, b] ** 2 - var) <= 4 * K * U, (K, B, c, b, rep[1, c, b] ** 2 - var)


# ---- 3. counter layout ---------------------------------------------------------------------------------------------------------------
def check_rows_are_one_row_calls(be):
    K, B, seed, offset = 257, 9, 77, 1234
    F = np.random.default_rng(4).random((4, K))
    full = _call(be, F, B, seed, offset=offset)
    Qd = (K + 3) // 4
    for c in range(4):
        one = _call(be, F[c:c + 1], B, seed, offset=offset + c * B * Qd)
        assert one["replicates"][:, 0].tobytes() == full["replicates"][:, c].tobytes(), c
        assert one["summary"][:, :, 0].tobytes() == full["summary"][:, :, c].tobytes(), c
    again = _call(be, F, B, seed, offset=offset)
    assert all(again[k].tobytes() == full[k].tobytes() for k in ("replicates", "summary"))
    for want in (("summary",), ("replicates",)):
        part = _call(be, F, B, seed, offset=offset, want=want)
        assert set(part) == set(want) | {"names"} and part[want[0]].tobytes() == full[want[0]].tobytes(), want
    other = _call(be, F, B, seed + 1, offset=offset)
    assert not np.array_equal(other["replicates"][0], full["replicates"][0])


def check_far_offsets(be):
    F = exact_rows(C=2, seed=6)
    assert_exact_against_host(be, F, 5, 0xABCDEF0123456789, 2 ** 40)
    assert_exact_against_host(be, F, 5, 0xABCDEF0123456789, 2 ** 32 - 3)          # the low counter word wraps inside replicate 0
    assert_exact_against_host(be, F, 5, 12, 2 ** 64 - 2 * 5 * 64)                  # the last counters there are


# ---- 4. routes -----------------------------------------------------------------------------------------------------------------------
def check_routes(be):
    F = ragged_fid(1000)
    a, b = (_call(be, F, 67, 5, offset=3, route=r) for r in ("lds", "global"))
    assert all(a[k].tobytes() == b[k].tobytes() for k in ("replicates", "summary"))
    assert np.isfinite(a["replicates"][:, 0]).all()
    try:
        _call(be, np.zeros((1, boot.LDS_MAX_K + 1)), 1, 0, route="lds")
    except ERRORS as e:
        assert "LDS" in str(e) or "lds" in str(e), e
    else:
        raise AssertionError("a forced LDS route above its cap was accepted")


# ---- 5. summary against NumPy on the backend's own replicates ---------------------------------------------------------------------
def check_summary_against_numpy(be):
    B = 400
    F = np.random.default_rng(8).beta(8.0, 2.0, (5, 128))
    res = _call(be, F, B, 31, conf=0.95)
    rep, s = res["replicates"], res["summary"]
    assert boot.ranks(B, 0.95) == (9, 390)
    for j in range(rep.shape[0]):
        for c in range(rep.shape[1]):
            x = rep[j, c]
            lo, hi = np.quantile(x, 0.025, method="lower"), np.quantile(x, 0.975, method="higher")
            assert s[j, 2, c] == lo == np.sort(x)[9] and s[j, 3, c] == hi == np.sort(x)[390], (j, c)
            assert s[j, 2, c] in x and s[j, 3, c] in x
            scale = np.abs(x).max()
            assert abs(s[j, 0, c] - math.fsum(x) / B) <= B * U * scale, (j, c)
            var = math.fsum((x - math.fsum(x) / B) ** 2) / (B - 1)
            assert abs(s[j, 1, c] ** 2 - var) <= 4 * B * U * max(1.0, scale ** 2), (j, c)
    assert np.all(s[0, 2] < s[0, 3]) and np.all(s[0, 1] > 0)


# ---- 6. statistics with teeth ------------------------------------------------------------------------------------------------------
STAT_SEED, STAT_C, STAT_K, STAT_B = 0x5EED000B, 200, 256, 400


def stat_fid():
    return np.random.default_rng(77).beta(8.0, 2.0, (STAT_C, STAT_K))


def stat_figures(be, F=None):
    """(rows whose 95 % interval of the mean fidelity covers 0.8, min and max over rows of SE / (std(f) / sqrt(K)))"""
    F = stat_fid() if F is None else F
    s = _call(be, F, STAT_B, STAT_SEED, want=("summary",))["summary"]
    covered = int(((1.0 - s[0, 3] <= 0.8) & (0.8 <= 1.0 - s[0, 2])).sum())
    ratio = s[0, 1] / (F.std(axis=1) / math.sqrt(STAT_K))
    return covered, float(ratio.min()), float(ratio.max())


def check_statistics(be):
    covered, lo, hi = stat_figures(be)
    assert covered >= 176, covered
    assert 0.85 <= lo and hi <= 1.15, (lo, hi)


ALL_CHECKS = (check_exact_permutation_rows, check_constant_row, check_two_valued_row, check_ragged, check_rows_are_one_row_calls,
              check_far_offsets, check_routes, check_summary_against_numpy, check_statistics)


# ---- the stand-in and its broken variants ----------------------------------------------------------------------------------------
BROKEN = ("zeros", "same_indices_every_replicate", "index_is_word_mod_K", "words_reversed_in_quad", "counter_ignores_row",
          "offset_ignored", "std_ddof1_in_replicate", "q_strictly_greater", "ranks_swapped")


class StandIn:
    """`backend.bootstrap_metrics` on the CPU through bootstrap.py; `broken`: one of BROKEN, a defect a check has to see"""

    def __init__(self, broken=None):
        assert broken is None or broken in BROKEN
        self.broken = broken

    def _indices(self, c, K, B, seed, offset):
        Qd, br = boot.quads(K), self.broken
        if br == "offset_ignored":
            offset = 0
        if br == "counter_ignores_row":
            c = 0
        if br is None or br in ("offset_ignored", "counter_ignores_row"):
            return boot.indices(1, K, B, seed, offset + c * B * Qd)[0]
        start = np.array([offset + (c * B + (0 if br == "same_indices_every_replicate" else b)) * Qd for b in range(B)], dtype=np.uint64)
        words = boot.philox4x32_10(start[:, None] + np.arange(Qd, dtype=np.uint64)[None, :], seed)          # (4, B, Q)
        if br == "words_reversed_in_quad":
            words = words[::-1]
        words = np.moveaxis(words, 0, -1).reshape(B, 4 * Qd)[:, :K].astype(np.uint64)
        if br == "index_is_word_mod_K":
            return (words % np.uint64(K)).astype(np.int64)
        return ((words * np.uint64(K)) >> np.uint64(32)).astype(np.int64)

    def bootstrap_metrics(self, fid, n_boot, seed, offset=0, q_thresholds=Q, conf=0.95, want=("summary", "replicates"), route="auto",
                          device=None):
        fid = np.asarray(fid, dtype=np.float64)
        C, K = fid.shape
        B, br = int(n_boot), self.broken
        thr = np.asarray(q_thresholds, dtype=np.float64).reshape(-1)
        if route == "lds" and K > boot.LDS_MAX_K:
            raise ValueError("route lds holds rows of at most %d values" % boot.LDS_MAX_K)
        if br in (None, "ranks_swapped"):
            rep = boot.replicates(fid, B, seed, offset, thr)
        else:
            rep = np.full((3 + thr.size, C, B), np.nan)
            for c in range(C):
                row = fid[c]
                if np.isnan(row).any():
                    continue
                m = row.sum() / K
                f = row[self._indices(c, K, B, seed, int(offset))]
                g = f - m
                mg = g.sum(axis=1) / K
                rep[0, c] = 1.0 - (m + mg)
                with np.errstate(invalid="ignore", divide="ignore"):
                    s2 = (g * g).sum(axis=1)
                    rep[1, c] = np.sqrt(np.maximum(0.0, (s2 - K * mg * mg) / (K - 1) if br == "std_ddof1_in_replicate" else s2 / K - mg * mg))
                rep[2, c] = f.min(axis=1)
                for i, t in enumerate(thr):
                    rep[3 + i, c] = ((f > t) if br == "q_strictly_greater" else (f >= t)).sum(axis=1) / K
            if br == "zeros":
                rep = np.zeros_like(rep)
        lo, hi = boot.ranks(B, conf)
        summ = boot.summary(rep, lo, hi)
        if br == "ranks_swapped":
            summ[:, (2, 3)] = summ[:, (3, 2)]
        res = {"replicates": rep, "summary": summ}
        res = {k: v for k, v in res.items() if k in want}
        res["names"] = boot.metric_names(thr.size)
        return res
