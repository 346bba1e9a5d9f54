"""Data-level checks of the stage that turns fidelities into the reported numbers: a reduction
`reduce(fid (C, K) float64, q_thresholds=..., dkw_eps=..., want_sorted=...) -> {"rim1", "std", "min" (3, C), "q" (3, nq, C), "sorted" (C, K)}`
and a p-RIM `rim_p(fid (C, K) float64, p) -> (C,)`, NumPy in and NumPy out: `backend.reduce_metrics` / `backend.rim_p` on the device
(reduce_kernel, reduce_rows_wave_kernel, rim_p_kernel, the row sort of csrc/k_reduce_sort.inc.h behind `enqueue_reduce`), the plain
NumPy implementation of tests/test_reduce_checks.py - and that file's broken stand-ins, each of which one of the checks must catch.

Known answers instead of random continuous data.  GRID DATA: fidelities j / 1024 (integer j in [0, 1024]), eps = 2^-6 = 16 grid steps,
thresholds on the grid, 0.0 and 1.0 among them.  On these `f - eps`, `f + eps`, both clips and every partial sum in any order are
exact in fp64 (K 1024 < 2^53), so the reference is INTEGER arithmetic and does not depend on route or summation order, and for all
three DKW variants
    rim1 == 1.0 - (S / K)   (S the exact sum: the two correctly rounded operations the kernels do)      min, q == count / K
hold bit for bit (np.array_equal); std is held to 1e-14 absolute against the exact rational variance (sum j, sum j^2 in Python
integers, the root by mpmath).  HIGH-FIDELITY GRID: f = 1 - j 2^-30, j < 1024, K <= 2^17: sums still exact, same exact comparisons;
the relative deviation of rim1 from the reference's gap formula (`oracle.wd_from_ideal`, which keeps RELATIVE accuracy where
1 - mean keeps absolute accuracy) is printed and returned, not asserted.  Rows sit on every comparison edge: at, one step below and
one above each threshold, the same after + eps and after - eps, below eps (lower clip), above 1 - eps (upper clip, counted against
the threshold 1.0), a constant row, the minimum as last element and in the last partial 64-lane / workgroup-wide slice.

NaN: a row holding ANY NaN - all of it, or one value (here the last) - gives NaN in rim1, std and min; its q is the count of the
non-NaN values >= thr over K (the reference's Q, `oracle.q_metric`), which is 0 for a whole-NaN row only.  Inside the variants the
device clamps NaN to 0 (fmin(fmax(NaN, 0), 1) = 0) where np.clip keeps NaN, so rows with a NaN are reduced with thresholds > 0.

The sort is compared with np.sort by np.array_equal (and must not turn +0.0 into -0.0); a row with a NaN comes back bit-identical.
p-RIM: relative bound (ceil(K / 512) + 6 + 7 + 4) 2^-52 max(1, 1/p) on the positive results against mpmath at 40 digits: the
per-thread chain, the wave tree, the waves in order, 4 ulp for the two pow calls and the division (HIP documents fp64 pow at 1 ulp).
The exponent of the outer power is the double 1.0 / p, as in the reference's `mean ** (1.0 / p)` and in the kernel: the bound has no
term for its rounding.  A case's inputs and reference are computed once per process and shared (read-only)."""
import math

import mpmath
import numpy as np

from oracle import robchar_oracle as orc

GRID = 1024
EPS = 2.0 ** -6
HF_SCALE = 2 ** 30
STD_TOL = 1e-14

THRESHOLDS = {0: ((),), 2: ((0.75, 1.0), (0.0, 0.953125)), 3: ((0.0, 0.5, 1.0),),
              8: ((0.0, 0.25, 0.5, 0.75, 0.953125, 0.96875, 0.984375, 1.0),)}
K_FEW = (1, 63, 64, 65, 2047, 2048, 2049, 4096, 4097, 8192, 8193, 10240, 10241, 16384, 16385, 20479, 20480, 20481, 100003)   # nq <= 2
K_MANY = (2048, 2049, 3584, 3585, 4095, 4096, 4097, 8193)                                                                    # nq > 2
HIGHFID_SHAPES = ((1000, 3), (1000, 70), (4097, 3), (10000, 3), (131072, 3))
HIGHFID_THR = (1.0 - 2.0 ** -21, 1.0)                # j = 512, j = 0

SORT_K = (1, 2, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 16383, 16384, 16385, 32768, 32769, 65536, 65537, 131072, 131073, 262144,
          262145, 524289)
SORT_PATTERNS = ("distinct", "eight", "constant", "ascending", "descending", "organ pipe", "zero one")
SORT_NAN_K = (1000, 16385, 262145)

RIMP_K = (1, 511, 512, 513, 10000, 100003)
RIMP_P = (0.5, 2, 2.5, 3, 7)
RIMP_C = (1, 5)

_CASES = {}
_SORT_CASES = {}


def ks_of(nq):
    return K_FEW if nq <= 2 else K_MANY


def cs_of(K):
    """up to 2048 values a row takes the workgroup route among fewer than 64 rows and the wave route among more"""
    return (3, 70) if K <= 2048 else (3,)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ------------------------------------------------------------------------------------------------------------------------
# grid rows (integers in units of 1 / scale, and a mask of the NaN positions) and the integer reference
# ------------------------------------------------------------------------------------------------------------------------


def edge_values(thr, scale=GRID, eps_i=16):
    """every grid value at which one of the kernel's comparisons changes: each threshold, the threshold shifted by -eps and by
    +eps, one step either side of all three; 0 .. eps + 1 (lower clip); 1 - eps - 1 .. 1 (upper clip)"""
    e = set(range(0, eps_i + 2)) | set(range(scale - eps_i - 1, scale + 1))
    for t in thr:
        ti = int(round(t * scale))
        e |= {ti + s + d for s in (0, -eps_i, eps_i) for d in (-1, 0, 1)}
    return np.array(sorted(v for v in e if 0 <= v <= scale), dtype=np.int64)


def mixed_row(rng, K, thr, lo=0):
    """half edge values, half any grid value, none below `lo`"""
    edge = edge_values(thr)
    row = np.where(rng.random(K) < 0.5, edge[rng.integers(0, edge.size, K)], rng.integers(0, GRID + 1, K))
    return np.maximum(row, lo)


def grid_row(kind, K, thr, seed):
    """0 edges   1 unique minimum in the last partial 64-lane slice   2 unique minimum last   3 constant, on a threshold
    4 unique minimum in the last partial slice of a 128- / 256- / 512-thread workgroup   5 above 1 - eps"""
    rng = np.random.default_rng([seed, kind, K])
    if kind == 0:
        return mixed_row(rng, K, thr)
    if kind == 3:
        return np.full(K, int(round(thr[(K + seed) % len(thr)] * GRID)) if len(thr) else 768, dtype=np.int64)
    if kind == 5:
        return rng.integers(GRID - 20, GRID + 1, K)
    row = mixed_row(rng, K, thr, lo=40)
    row[{1: ((K - 1) // 64) * 64, 2: K - 1, 4: ((K - 1) // 128) * 128}[kind]] = (3, 5, 7)[kind // 2]      # below eps: clipped at 0
    return row


def grid_slab(K, C, thr, part):
    """C = 3: part 0 = kinds 0 1 2, part 1 = kinds 3 4 5; more rows: the six kinds in turn"""
    J = np.stack([grid_row((3 * part + r) % 6, K, thr, r) for r in range(C)])
    return J, np.zeros(J.shape, dtype=bool)


def nan_slab(K, C, thr):
    """rows in turn: all NaN; edge values with a single NaN as last element; edge values"""
    J = np.stack([grid_row(0, K, thr, 100 + r) for r in range(C)])
    nan = np.zeros(J.shape, dtype=bool)
    nan[0::3] = True
    nan[1::3, K - 1] = True
    return J, nan


def highfid_slab(K, C):
    """f = 1 - j 2^-30: any j < 1024; j around the threshold j = 512; exactly 1.0 (rim1 = 0); then again"""
    rng = np.random.default_rng([30, K, C])
    j = rng.integers(0, 1024, (C, K))
    j[1::3] = rng.integers(510, 515, j[1::3].shape)
    j[2::3] = 0
    return HF_SCALE - j, np.zeros(j.shape, dtype=bool)


def to_float(J, nan, scale):
    F = J / float(scale)                                        # exact: a power of two
    F[nan] = np.nan
    return F


def reference(J, nan, scale, eps_i, thr):
    C, K = J.shape
    bad = nan.any(axis=1)
    ref = {"rim1": np.full((3, C), np.nan), "std": np.full((3, C), np.nan), "min": np.full((3, C), np.nan),
           "q": np.empty((3, len(thr), C))}
    tis = [int(round(t * scale)) for t in thr]
    assert all(ti / scale == t for ti, t in zip(tis, thr))
    for v, shift in enumerate((0, -eps_i, eps_i)):
        Jv = np.clip(J + shift, 0, scale)
        S = Jv.sum(axis=1)
        assert int(S.max()) < 2 ** 53
        ref["rim1"][v] = np.where(bad, np.nan, 1.0 - (S / float(scale)) / K)
        ref["min"][v] = np.where(bad, np.nan, Jv.min(axis=1) / float(scale))
        for j, ti in enumerate(tis):
            ref["q"][v, j] = ((Jv >= ti) & ~nan).sum(axis=1) / K
        d = Jv - Jv.min(axis=1, keepdims=True)                  # the variance does not move with the row
        s1, s2 = d.sum(axis=1), (d * d).sum(axis=1)
        for c in np.flatnonzero(~bad):
            num = K * int(s2[c]) - int(s1[c]) ** 2
            ref["std"][v, c] = float(mpmath.sqrt(mpmath.mpf(num) / (K * K * scale * scale)))
    return ref


def case(key, make, scale, eps_i, thr):
    """(F, thresholds, reference) of a named slab, computed once; `make` -> (J, nan)"""
    if key not in _CASES:
        with mpmath.workdps(40):
            J, nan = make()
            F = to_float(J, nan, scale)
            ref = reference(J, nan, scale, eps_i, thr)
        _frozen(F, *ref.values())
        _CASES[key] = (F, np.array(thr, dtype=np.float64), ref)
    return _CASES[key]


def compare(got, ref, tag):
    """rim1, min and q bit for bit, std to STD_TOL; -> the largest std error"""
    for name in ("rim1", "min", "q"):
        g = np.asarray(got[name])
        assert g.shape == ref[name].shape and g.dtype == np.float64, (tag, name, g.shape, g.dtype)
        assert np.array_equal(g, ref[name], equal_nan=True), (tag, name, g, ref[name])
    g, e = np.asarray(got["std"]), ref["std"]
    assert g.shape == e.shape and np.array_equal(np.isnan(g), np.isnan(e)), (tag, "std", g, e)
    err = float(np.max(np.abs(np.where(np.isnan(e), 0.0, g - e)), initial=0.0))
    assert err <= STD_TOL, (tag, "std", err)
    return err


# ------------------------------------------------------------------------------------------------------------------------
# reduction checks
# ------------------------------------------------------------------------------------------------------------------------


def grid_cases(nq, K, C):
    """the slabs of one shape: per threshold set the grid rows (both halves when C = 3) and the rows with NaN"""
    for ti, thr in enumerate(THRESHOLDS[nq]):
        for part in ((0, 1) if C < 6 else (0,)):
            yield ("grid", K, C, nq, ti, part), case(("grid", K, C, nq, ti, part), lambda: grid_slab(K, C, thr, part), GRID, 16, thr)
        pos = tuple(t if t > 0 else 1.0 / GRID for t in thr)
        yield ("nan", K, C, nq, ti), case(("nan", K, C, nq, ti), lambda: nan_slab(K, C, pos), GRID, 16, pos)


def check_grid(reduce, nqs=(0, 2, 3, 8), ks=None, cs=None):
    """every branch of the routing at both sides of every boundary; -> the largest std error"""
    worst = 0.0
    for nq in nqs:
        for K in (ks_of(nq) if ks is None else ks):
            for C in (cs_of(K) if cs is None else cs):
                for tag, (F, thr, ref) in grid_cases(nq, K, C):
                    worst = max(worst, compare(reduce(F.copy(), q_thresholds=thr, dkw_eps=EPS), ref, tag))
    print(f"reduce_checks.check_grid nq={tuple(nqs)}: worst |std - exact| = {worst:.3e} (bound {STD_TOL:.0e})")
    return worst


def check_nan_rows(reduce):
    """what the header says of rows with a NaN, spelled out on one slab per route: both kinds give NaN in rim1 / std / min; the
    whole-NaN row counts 0, the row with one NaN counts its other values"""
    for nq, K, C in ((2, 100, 3), (2, 100, 70), (8, 2048, 3), (2, 5000, 3), (8, 5000, 3), (2, 20481, 3)):
        for tag, (F, thr, ref) in grid_cases(nq, K, C):
            if tag[0] != "nan":
                continue
            assert np.isnan(F[0]).all() and np.isnan(F[1]).sum() == 1 and np.isnan(F[1, -1]) and not np.isnan(F[2]).any()
            assert (ref["q"][:, :, 0] == 0).all() and (ref["q"][:, :, 1].max(axis=0) > 0).all() and np.isnan(ref["rim1"][:, :2]).all()
            for v, data in enumerate((F, np.clip(F - EPS, 0, 1), np.clip(F + EPS, 0, 1))):
                for j, t in enumerate(thr):
                    assert ref["q"][v, j, 1] == orc.q_metric(data[1], t)
            compare(reduce(F.copy(), q_thresholds=thr, dkw_eps=EPS), ref, tag)


def check_alone(reduce, cases=None):
    """above 2048 values a row's bits do not depend on the rows reduced with it (include/robchar_hip.h)"""
    if cases is None:
        cases = [(nq, K) for nq in (2, 8) for K in ks_of(nq) if K > 2048]
    for nq, K in cases:
        F, thr, ref = case(("grid", K, 3, nq, 0, 0), lambda: grid_slab(K, 3, THRESHOLDS[nq][0], 0), GRID, 16, THRESHOLDS[nq][0])
        among = reduce(F.copy(), q_thresholds=thr, dkw_eps=EPS)
        alone = reduce(F[1:2].copy(), q_thresholds=thr, dkw_eps=EPS)
        for name in ("rim1", "std", "min", "q"):
            a, b = np.asarray(alone[name]), np.asarray(among[name])
            assert np.ascontiguousarray(a[..., 0]).tobytes() == np.ascontiguousarray(b[..., 1]).tobytes(), (nq, K, name)


def check_highfid(reduce, shapes=HIGHFID_SHAPES):
    """-> the largest relative deviation of rim1 from `oracle.wd_from_ideal` (printed, not asserted)"""
    worst_dev, worst_std = 0.0, 0.0
    for K, C in shapes:
        F, thr, ref = case(("highfid", K, C), lambda: highfid_slab(K, C), HF_SCALE, 2 ** 24, HIGHFID_THR)
        got = reduce(F.copy(), q_thresholds=thr, dkw_eps=EPS)
        worst_std = max(worst_std, compare(got, ref, ("highfid", K, C)))
        assert (np.asarray(got["rim1"])[0, 2::3] == 0.0).all() and (np.asarray(got["rim1"])[2] == 0.0).all()
        for c in range(min(C, 6)):
            gap = orc.wd_from_ideal(F[c].copy())
            if gap > 0:
                worst_dev = max(worst_dev, abs(float(np.asarray(got["rim1"])[0, c]) - gap) / gap)
    print(f"reduce_checks.check_highfid: worst relative deviation of rim1 = 1 - mean from wd_from_ideal = {worst_dev:.3e}; "
          f"worst |std - exact| = {worst_std:.3e}")
    return worst_dev


# ------------------------------------------------------------------------------------------------------------------------
# row sort
# ------------------------------------------------------------------------------------------------------------------------


def sort_rows(K, pattern):
    rng = np.random.default_rng([SORT_PATTERNS.index(pattern), K])
    up = np.arange(K, dtype=np.float64)
    rows = {"distinct": lambda r: rng.random(K),
            "eight": lambda r: rng.integers(0, 8, K) / 8.0,
            "constant": lambda r: np.full(K, 0.25 * (r + 1)),
            "ascending": lambda r: (up + r) / (K + 2),
            "descending": lambda r: (up[::-1] + r) / (K + 2),
            "organ pipe": lambda r: np.minimum(up + r, K - 1 - up) / K,
            "zero one": lambda r: rng.integers(0, 2, K).astype(np.float64)}[pattern]
    return np.stack([rows(r) for r in range(3)])


def sort_case(K, pattern):
    """(F, np.sort(F)); the cases of one K at a time are kept (the longest slab is 12.6 MB)"""
    if _SORT_CASES and next(iter(_SORT_CASES))[0] != K:
        _SORT_CASES.clear()
    if (K, pattern) not in _SORT_CASES:
        F = np.ascontiguousarray(sort_rows(K, pattern))
        _SORT_CASES[(K, pattern)] = _frozen(F, np.sort(F, axis=1))
    return _SORT_CASES[(K, pattern)]


def check_sort(reduce, ks=SORT_K, patterns=SORT_PATTERNS):
    for K in ks:
        for pattern in patterns:
            F, want = sort_case(K, pattern)
            if pattern == "distinct" and K > 1:
                assert (np.diff(want, axis=1) > 0).all()
            got = np.asarray(reduce(F.copy(), want_sorted=True)["sorted"])
            assert got.shape == want.shape and got.dtype == np.float64, (K, pattern)
            assert np.array_equal(got, want), (K, pattern)
            assert not np.signbit(got).any(), (K, pattern)


def check_sort_nan(reduce, ks=SORT_NAN_K):
    """one K per route: a whole-NaN row and a row with one NaN come back bit-identical, the row between them sorted"""
    for K in ks:
        if ("sort nan", K) not in _CASES:
            F = np.random.default_rng([9, K]).random((4, K))
            F[0] = np.nan
            F[2, K // 2] = np.nan
            _CASES[("sort nan", K)] = _frozen(F)[0]
        F = _CASES[("sort nan", K)]
        got = np.asarray(reduce(F.copy(), want_sorted=True)["sorted"])
        for c in (0, 2):
            assert got[c].tobytes() == F[c].tobytes(), (K, c)
        for c in (1, 3):
            assert np.array_equal(got[c], np.sort(F[c])), (K, c)


# ------------------------------------------------------------------------------------------------------------------------
# p-RIM
# ------------------------------------------------------------------------------------------------------------------------


def rimp_bound(K, p):
    return (math.ceil(K / 512) + 6 + 7 + 4) * 2.0 ** -52 * max(1.0, 1.0 / p)


def rimp_rows(K, C, which):
    """(u, scale, kind) per row with 1 - f = u / scale: "grid", "highfid", "ones" (result 0.0), "nan", "above" = a grid row with one
    value 1 + 2^-52 (inside the reference's range guard; 1 - f = -2^-52).  C = 1: the grid row or the high-fidelity row."""
    rng = np.random.default_rng([77, K, C, which])
    kinds = ("grid", "highfid", "ones", "nan", "above") if C == 5 else (("grid", "highfid")[which],)
    rows = []
    for kind in kinds:
        if kind == "highfid":
            rows.append((rng.integers(0, 1024, K), HF_SCALE, kind))
        elif kind == "ones":
            rows.append((np.zeros(K, dtype=np.int64), GRID, kind))
        else:
            rows.append((rng.integers(0, GRID + 1, K), GRID, kind))
    return rows


def rimp_case(K, C, which, p):
    """(F, reference per row: mpmath number, 0 or NaN), F shared by every p"""
    fkey = ("rimp", K, C, which)
    if fkey not in _CASES:
        rows = rimp_rows(K, C, which)
        F = np.stack([1.0 - u / float(scale) for u, scale, _ in rows])           # exact
        for c, (_, _, kind) in enumerate(rows):
            if kind == "nan":
                F[c] = np.nan
            if kind == "above":
                F[c, K // 2] = 1.0 + 2.0 ** -52
        _CASES[fkey] = (_frozen(F)[0], rows)
    F, rows = _CASES[fkey]
    key = fkey + (p,)
    if key not in _CASES:
        with mpmath.workdps(40):
            ref = []
            for u, scale, kind in rows:
                if kind == "nan":
                    ref.append(mpmath.nan)
                    continue
                cnt = np.bincount(u, minlength=1)
                if kind == "above":
                    cnt[u[K // 2]] -= 1
                pw = int(p) if float(p).is_integer() else mpmath.mpf(p)
                total = mpmath.fsum(int(n) * (mpmath.mpf(int(v)) / scale) ** pw for v, n in enumerate(cnt) if n and v)
                if kind == "above":
                    total = total + (-mpmath.mpf(2) ** -52) ** pw if float(p).is_integer() else mpmath.nan
                mean = total / K
                # a negative mean (K = 1, odd p) has no real root: NumPy gives NaN.  The exponent is the double 1.0 / p.
                ref.append(mpmath.nan if mpmath.isnan(mean) or mean < 0 else mean ** mpmath.mpf(1.0 / p) if mean > 0 else mpmath.mpf(0))
        _CASES[key] = tuple(ref)
    return F, _CASES[key]


def check_rim_p(rim_p, ks=RIMP_K, ps=RIMP_P, cs=RIMP_C):
    """-> the largest ratio of the relative error to its bound"""
    worst = 0.0
    for K in ks:
        for C in cs:
            for which in ((0, 1) if C == 1 else (0,)):
                for p in ps:
                    F, ref = rimp_case(K, C, which, p)
                    got = np.asarray(rim_p(F.copy(), p))
                    assert got.shape == (C,) and got.dtype == np.float64, (K, C, p)
                    with np.errstate(invalid="ignore"):
                        plain = np.power(1.0 - F, p).mean(axis=1) ** (1.0 / p)   # the reference's formula (wd...py:147-174)
                    with mpmath.workdps(40):
                        for c, (g, e) in enumerate(zip(got.tolist(), ref)):
                            assert math.isnan(g) == math.isnan(plain[c]) == bool(mpmath.isnan(e)), (K, C, p, c, g, plain[c])
                            if mpmath.isnan(e):
                                continue
                            if e == 0:
                                assert g == 0.0, (K, C, p, c, g)
                                continue
                            ratio = float(abs(mpmath.mpf(g) - e) / e) / rimp_bound(K, p)
                            worst = max(worst, ratio)
                            assert ratio <= 1.0, (K, C, p, c, g, float(e), ratio)
    print(f"reduce_checks.check_rim_p K={tuple(ks)}: worst relative error / bound = {worst:.3f}")
    return worst


REDUCE_CHECKS = (check_grid, check_nan_rows, check_alone, check_highfid, check_sort, check_sort_nan)
