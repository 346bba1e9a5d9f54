"""The checks of tests/reduce_checks.py have teeth: they pass on a plain NumPy reduction, row sort and p-RIM written here (the two
correctly rounded operations of rim1 = 1 - sum / K, the two-pass population std, np.sort with NaN rows copied through), and each of
fourteen broken variants fails the check that is there for it.  CPU only.  (`stand_in.reduce_metrics` is not used: it computes rim1
by the gap formula and differs from 1 - mean in the last bits.)"""
import warnings

import numpy as np
import pytest

import reduce_checks as rc


def reduce_numpy(broken=None):
    """the reduction with one defect:
        ">"            counts f > thr                                "threshold first"  counts the unshifted value in every variant
        "no lower clip" clip(f - eps) without the clip at 0          "last dropped"     the last element of a row left out
        "centre min"   min of the variants = min of the centre      "ddof"             std with K - 1
        "float32"      sums accumulated in float32                   "nanmean"          a single NaN ignored by the mean
        "q zero"       q = 0 on every row that holds a NaN           "ties collapsed"   sort = np.unique padded with the maximum
        "beyond chunk" elements beyond 16 384 left unsorted          "nan sorted"       NaN rows sorted instead of copied through"""
    def reduce(fid, q_thresholds=(0.95, 0.98), dkw_eps=0.0, want_sorted=False):
        F = np.asarray(fid, dtype=np.float64)
        C, K = F.shape
        thr = np.asarray(q_thresholds, dtype=np.float64).reshape(-1)
        bad = np.isnan(F).any(axis=1)
        low = F - dkw_eps if broken == "no lower clip" else np.maximum(F - dkw_eps, 0.0)
        res = {"rim1": np.empty((3, C)), "std": np.empty((3, C)), "min": np.empty((3, C)), "q": np.empty((3, thr.size, C))}
        for v, data in enumerate((F, np.minimum(low, 1.0), np.clip(F + dkw_eps, 0.0, 1.0))):
            used = data[:, :K - 1] if broken == "last dropped" and K > 1 else data
            if broken == "float32":
                mean = used.astype(np.float32).sum(axis=1, dtype=np.float32).astype(np.float64) / K
            elif broken == "nanmean":
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore", RuntimeWarning)
                    mean = np.nanmean(used, axis=1)
            else:
                mean = used.sum(axis=1) / K
            res["rim1"][v] = 1.0 - mean
            res["std"][v] = np.sqrt(((used - mean[:, None]) ** 2).sum(axis=1) / (K - 1 if broken == "ddof" else K))
            res["min"][v] = (F if broken == "centre min" else used).min(axis=1)
            counted = F[:, :used.shape[1]] if broken == "threshold first" else used
            for j, t in enumerate(thr):
                res["q"][v, j] = ((counted > t) if broken == ">" else (counted >= t)).sum(axis=1) / K
            if broken == "q zero":
                res["q"][v][:, bad] = 0.0
        if want_sorted:
            ok = slice(None) if broken == "nan sorted" else ~bad
            srt = F.copy()
            srt[ok] = np.sort(F[ok], axis=1)
            if broken == "beyond chunk":
                srt[ok] = F[ok]
                srt[ok, :16384] = np.sort(F[ok, :16384], axis=1)
            if broken == "ties collapsed":
                for c in np.flatnonzero(~bad):
                    u = np.unique(F[c])
                    srt[c] = np.concatenate([u, np.full(K - u.size, u[-1])])
            res["sorted"] = srt
        return res
    return reduce


def rim_p_numpy(broken=None):
    """`oracle.rim_p` per row, with "row 0" (every row computed from row 0) or "abs" (|1 - f|)"""
    def rim_p(fid, p):
        F = np.asarray(fid, dtype=np.float64)
        if broken == "row 0":
            F = np.broadcast_to(F[:1], F.shape)
        d = np.abs(1.0 - F) if broken == "abs" else 1.0 - F
        with np.errstate(invalid="ignore"):
            return np.power(d, p).mean(axis=1) ** (1.0 / p)
    return rim_p


@pytest.mark.parametrize("nq", [0, 2, 3, 8])
def test_grid_rows_every_shape(nq):
    rc.check_grid(reduce_numpy(), nqs=(nq,))


@pytest.mark.parametrize("check", [rc.check_nan_rows, rc.check_alone, rc.check_highfid, rc.check_sort_nan], ids=lambda c: c.__name__)
def test_numpy_reduction_passes(check):
    check(reduce_numpy())


@pytest.mark.parametrize("K", rc.SORT_K)
def test_numpy_sort_passes(K):
    rc.check_sort(reduce_numpy(), ks=(K,))


@pytest.mark.parametrize("K", rc.RIMP_K)
def test_numpy_rim_p_passes(K):
    rc.check_rim_p(rim_p_numpy(), ks=(K,))


def test_the_rows_hold_what_they_are_there_for():
    """every edge the module promises is in the data: values at, below and above each threshold, before and after either shift; both
    clips; the minimum where it is said to be; one NaN last"""
    thr = rc.THRESHOLDS[8][0]
    for K in (2049, 20481):
        (F, _, ref), = [c for t, c in rc.grid_cases(8, K, 3) if t[0] == "grid" and t[-1] == 0]
        j = np.rint(F * rc.GRID).astype(int)
        assert np.array_equal(j / rc.GRID, F)
        for t in thr:
            ti = int(t * rc.GRID)
            for shift in (0, -16, 16):
                for d in (-1, 0, 1):
                    if 0 <= ti + shift + d <= rc.GRID:
                        assert (j[0] == ti + shift + d).any(), (t, shift, d)
        assert (j[0] < 16).any() and (j[0] > rc.GRID - 16).any()
        assert j[1].argmin() == ((K - 1) // 64) * 64 and (j[1] == j[1].min()).sum() == 1 and j[1].min() < 16
        assert j[2].argmin() == K - 1 and (j[2] == j[2].min()).sum() == 1
        (F, _, _), = [c for t, c in rc.grid_cases(8, K, 3) if t[0] == "grid" and t[-1] == 1]
        j = np.rint(F * rc.GRID).astype(int)
        assert (j[0] == j[0, 0]).all() and j[0, 0] / rc.GRID in thr
        assert j[1].argmin() == ((K - 1) // 128) * 128 >= ((K - 1) // 512) * 512 and (j[1] == j[1].min()).sum() == 1
        assert (j[2] >= rc.GRID - 20).all() and (j[2] == rc.GRID).any()


GRID_SMALL = {"nqs": (2,), "ks": (65,), "cs": (3,)}


@pytest.mark.parametrize("broken, check, kwargs", [
    (">", rc.check_grid, GRID_SMALL),
    ("threshold first", rc.check_grid, GRID_SMALL),
    ("no lower clip", rc.check_grid, GRID_SMALL),
    ("last dropped", rc.check_grid, GRID_SMALL),
    ("centre min", rc.check_grid, GRID_SMALL),
    ("ddof", rc.check_grid, GRID_SMALL),
    ("float32", rc.check_grid, {"nqs": (2,), "ks": (100003,)}),
    ("nanmean", rc.check_nan_rows, {}),
    ("q zero", rc.check_nan_rows, {}),
    ("ties collapsed", rc.check_sort, {"ks": (1025,), "patterns": ("eight",)}),
    ("beyond chunk", rc.check_sort, {"ks": (16385,), "patterns": ("distinct",)}),
    ("nan sorted", rc.check_sort_nan, {"ks": (1000,)}),
])
def test_broken_reduction_fails_its_check(broken, check, kwargs):
    with pytest.raises(AssertionError):
        check(reduce_numpy(broken), **kwargs)


@pytest.mark.parametrize("broken, kwargs", [("row 0", {"ks": (513,), "cs": (5,)}), ("abs", {"ks": (513,), "cs": (5,), "ps": (2.5,)})])
def test_broken_rim_p_fails_its_check(broken, kwargs):
    with pytest.raises(AssertionError):
        rc.check_rim_p(rim_p_numpy(broken), **kwargs)


def test_each_defect_is_caught_by_its_own_field():
    """the stand-ins are wrong in ONE thing: on the same slab the other fields still hold"""
    (F, thr, ref), = [c for t, c in rc.grid_cases(2, 2049, 3) if t[0] == "grid" and t[-1] == 0 and t[4] == 0]
    wrong = {">": {"q"}, "threshold first": {"q"}, "no lower clip": {"rim1", "std", "min"},
             "centre min": {"min"}, "ddof": {"std"}}
    for broken, fields in wrong.items():
        got = reduce_numpy(broken)(F.copy(), q_thresholds=thr, dkw_eps=rc.EPS)
        for name in ("rim1", "std", "min", "q"):
            same = np.allclose(got[name], ref[name], atol=rc.STD_TOL, rtol=0) if name == "std" else np.array_equal(got[name], ref[name])
            assert same == (name not in fields), (broken, name)


def test_stand_ins_pass_where_their_defect_does_not_show():
    rc.check_grid(reduce_numpy("float32"), **GRID_SMALL)                             # 65 * 1024 < 2^24: float32 sums are exact
    rc.check_sort(reduce_numpy("beyond chunk"), ks=(16384,), patterns=("distinct", "eight"))
    rc.check_sort(reduce_numpy("ties collapsed"), ks=(1025,), patterns=("distinct", "ascending"))
    rc.check_sort(reduce_numpy("nan sorted"), ks=(1025,))
    rc.check_rim_p(rim_p_numpy("abs"), ks=(513,), ps=(2, 7))
    rc.check_rim_p(rim_p_numpy("row 0"), ks=(513,), cs=(1,))
