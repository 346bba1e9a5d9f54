"""Checks of the BOXED batched L-BFGS state machine (box bounds lo <= x <= hi, projected steps; the rules are in lbfgs.py) with
analytic objectives evaluated on the host, written against any MACHINE: the definition (`lbfgs.LBFGS.init(x0, mask, lo, hi)`), the
device kernels behind `backend.lbfgs_init / lbfgs_advance(bounds=...)` (tests/test_gpu_lbfgs_box.py wraps them) and the broken
stand-ins of tests/test_lbfgs_box_checks.py, each of which one of the checks must catch.

A machine is made by `factory(x0, mask, lo, hi, **params)` and has `advance(ft, gt)`, `state_array()` and, as NumPy arrays refreshed
by every call, `trial`, `x`, `f`, `g`, `status`, `iters`, `evals`, `count` (the fields of `lbfgs.LBFGS`)."""
import itertools

import numpy as np

import lbfgs_checks as lc

lbfgs = lc.lbfgs


def definition(x0, mask=None, lo=None, hi=None, **params):
    return lbfgs.LBFGS(**params).init(x0, mask, lo, hi)


def project(v, lo, hi):
    return np.where(v < lo, lo, np.where(v > hi, hi, v))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def separable(a, c):
    """f = 1/2 sum_i a_i (x_i - c_i)^2 per row; a, c (C, n) or (n,)"""
    def fun(x):
        r = x - c
        return 0.5 * (a * r * r).sum(axis=1), a * r
    return fun


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
SEP_C, SEP_N, SEP_LO, SEP_HI, SEP_GTOL = 65, 8, -1.0, 1.5, 1e-9


def check_separable(factory):
    """a separable quadratic in the box [-1, 1.5]^8, 65 rows: every row ends with status 1; a coordinate whose minimiser c_i lies
    outside the box equals the bound bit for bit; the others are within gtol / min a of c_i (|a_i (x_i - c_i)| <= gtol there: the
    projected gradient of an interior coordinate is its gradient, as |g_i| <= gtol is far below the distance to a bound, and a
    coordinate ON a bound with c_i inside has |g_i| = a_i |bound - c_i|, which the projected gradient sees in full)"""
    rng = np.random.default_rng(2024)
    a = np.exp(rng.uniform(-1.0, 1.5, (SEP_C, SEP_N)))
    c = rng.uniform(-3.0, 3.0, (SEP_C, SEP_N))
    x0 = rng.uniform(-2.0, 2.5, (SEP_C, SEP_N))                       # some starts outside the box
    mc = factory(x0, None, SEP_LO, SEP_HI, gtol=SEP_GTOL, maxiter=200)
    calls = lc.drive(mc, separable(a, c), 400)
    assert (mc.status == 1).all(), (mc.status, calls)
    below, above = c < SEP_LO, c > SEP_HI
    assert below.sum() > 50 and above.sum() > 50 and (~below & ~above).sum() > 50
    assert np.array_equal(bits(mc.x[below]), bits(np.full(below.sum(), SEP_LO))), "a coordinate pushed below the box is not ON lo"
    assert np.array_equal(bits(mc.x[above]), bits(np.full(above.sum(), SEP_HI))), "a coordinate pushed above the box is not ON hi"
    inside = ~below & ~above
    err = np.abs(mc.x - c)[inside].max()
    print("separable: calls", calls, "worst error inside", err)
    assert err <= SEP_GTOL / np.exp(-1.0), err                         # 2.72e-9
    assert np.isnan(mc.trial).all()
    return calls


def kkt_reference(A, xs, lo, hi):
    """the minimiser of 1/2 (x - xs)^T A (x - xs) in the box by enumeration of all 3^n active sets: per variable on lo, on hi or
    free; solve the reduced system, keep the feasible one whose multipliers have the right signs"""
    n = len(xs)
    found = []
    for pattern in itertools.product((0, 1, 2), repeat=n):            # 0 free, 1 on lo, 2 on hi
        pattern = np.array(pattern)
        free = pattern == 0
        x = np.where(pattern == 1, lo, np.where(pattern == 2, hi, 0.0))
        if not np.isfinite(x[~free]).all():
            continue
        if free.any():
            rhs = (A @ xs)[free] - A[np.ix_(free, ~free)] @ x[~free]
            x[free] = np.linalg.solve(A[np.ix_(free, free)], rhs)
        g = A @ (x - xs)
        ok = (x >= lo - 1e-13).all() and (x <= hi + 1e-13).all()
        ok = ok and (g[pattern == 1] >= -1e-12).all() and (g[pattern == 2] <= 1e-12).all()
        if ok:
            found.append(x)
    assert found, "no KKT point found"
    for x in found[1:]:                                               # (degenerate patterns give the same point)
        assert np.abs(x - found[0]).max() <= 1e-9
    return found[0]


def check_coupled(factory):
    """coupled SPD quadratics (condition 30, smallest eigenvalue 1), n = 3 and 4, in boxes that cut the minimiser off: every row
    ends with status 1 at the KKT point of the enumeration, to gtol * cond.  (gtol = 1e-7: the value at a constrained minimum
    is of order 0.1 .. 1, so a decrease is resolved to ~1e-17 .. 1e-16 and with it |g| to ~1e-8 only - the line search cannot
    see further; lbfgs_checks.check_mask has the same limit.  One decade above that.)"""
    gtol, cond = 1e-7, 30.0
    for n in (3, 4):
        fun, xs, A = lc.quadratic(n, seed=40 + n, cond=cond)
        rng = np.random.default_rng(n)
        C = 6
        lo = xs - rng.uniform(-0.5, 1.0, (C, n))                      # lo above the minimiser where the draw is negative
        hi = lo + rng.uniform(0.2, 1.5, (C, n))
        x0 = xs + rng.standard_normal((C, n))
        mc = factory(x0, None, lo, hi, gtol=gtol, maxiter=300)
        calls = lc.drive(mc, fun, 600)
        assert (mc.status == 1).all(), (n, mc.status, calls)
        on_bound = 0
        for c in range(C):
            want = kkt_reference(A, xs, lo[c], hi[c])
            on_bound += int(((want == lo[c]) | (want == hi[c])).sum())
            assert np.abs(mc.x[c] - want).max() <= gtol * cond, (n, c, mc.x[c], want)
        assert on_bound >= C, "the boxes cut nothing off: the case is vacuous"


def smooth_objective(n, seed):
    """1 - mean of three 'fidelities' 1 / (1 + q_k(x)) (lbfgs_checks.sample_rows): smooth, not convex"""
    rows = lc.sample_rows(n, seed)

    def fun(x):
        mean, _ = rows(x)
        return 1.0 - mean[:, 0], -mean[:, 1:]
    return fun


def check_invariants(factory):
    """random smooth objectives, n = 3, 8, 13, rows with own boxes (some sides infinite): after every call lo <= trial <= hi and
    lo <= x <= hi exactly, f never increases, a done row stays frozen and its trial row is NaN; bounds are reached on the way"""
    for n in (3, 8, 13):
        fun = smooth_objective(n, 7 * n)
        rng = np.random.default_rng(100 + n)
        C = 12
        lo = rng.uniform(-0.6, 0.0, (C, n))
        hi = lo + rng.uniform(0.05, 0.8, (C, n))
        lo[rng.random((C, n)) < 0.15] = -np.inf
        hi[rng.random((C, n)) < 0.15] = np.inf
        x0 = rng.uniform(-1.0, 1.0, (C, n))
        mc = factory(x0, None, lo, hi, gtol=1e-7, maxiter=40, m=3)
        assert (mc.trial >= lo).all() and (mc.trial <= hi).all()
        frozen, touched, calls = {}, 0, 0
        f_before = None
        while (mc.status == 0).any() and calls < 150:
            was_done = mc.status != 0
            mc.advance(*fun(mc.trial))
            calls += 1
            live = mc.status == 0
            assert (mc.trial[live] >= lo[live]).all() and (mc.trial[live] <= hi[live]).all(), (n, calls, "trial outside the box")
            assert (mc.x >= lo).all() and (mc.x <= hi).all(), (n, calls, "x outside the box")
            assert np.isnan(mc.trial[~live]).all(), (n, calls, "a done row's trial row is not NaN")
            if f_before is not None:
                assert (mc.f <= f_before).all(), (n, calls, "a value went up")
            f_before = mc.f.copy()
            snap = mc.state_array()
            for c in np.nonzero(~live)[0]:
                if was_done[c]:
                    assert np.array_equal(snap[:, c], frozen[c], equal_nan=True), (n, calls, c, "a done row changed")
                frozen[c] = snap[:, c].copy()
            touched += int(((mc.x == lo) | (mc.x == hi)).sum())
        assert touched > 0 and (mc.iters >= 1).sum() >= C - 2, (n, touched, mc.iters)     # (a row may start at a KKT corner)
        assert (mc.status != 0).all() and (mc.status != 5).all(), (n, mc.status)


def check_start_rows(factory):
    """a start outside the box is projected; a variable that starts ON a bound with an inward gradient leaves it; one that starts on
    a bound with an outward gradient stays there (bit for bit, in every trial point) while the other variables move"""
    a = np.array([1.0, 2.0, 0.5, 3.0])
    c = np.array([0.3, 0.25, -2.0, 5.0])                               # minimisers: inside, inside, below lo, above hi
    lo, hi = np.full(4, -1.0), np.full(4, 1.0)
    x0 = np.array([[5.0, -1.0, -1.0, 0.0],                             # outside; on lo, inward; on lo, outward; free
                   [-7.0, 1.0, 0.5, 1.0]])                             # outside; on hi, inward; free; on hi, outward
    mc = factory(x0, None, lo, hi, gtol=1e-10, maxiter=100)
    assert np.array_equal(bits(mc.trial), bits(project(x0, lo, hi))) and np.array_equal(bits(mc.x), bits(mc.trial))
    fun = separable(a, c)
    calls = 0
    while (mc.status == 0).any() and calls < 200:
        mc.advance(*fun(mc.trial))
        calls += 1
        live = mc.status == 0
        if live[0]:
            assert mc.trial[0, 2] == -1.0, "row 0: the variable with the outward gradient left lo"
        if live[1]:
            assert mc.trial[1, 3] == 1.0, "row 1: the variable with the outward gradient left hi"
    assert (mc.status == 1).all(), (mc.status, calls)
    want = project(np.broadcast_to(c, (2, 4)), lo, hi)
    assert np.abs(mc.x - want).max() <= 1e-9, mc.x
    assert mc.x[0, 1] != -1.0 and mc.x[1, 1] != 1.0, "a variable on a bound with an inward gradient stayed there"
    assert mc.x[0, 2] == -1.0 and mc.x[0, 3] == 1.0 and mc.x[1, 2] == -1.0 and mc.x[1, 3] == 1.0


def check_lo_equals_hi(factory):
    """lo == hi on a variable behaves like a mask: the variable is that value in every trial point, the free ones reach the minimum
    of the restricted problem"""
    n = 5
    fun, xs, A = lc.quadratic(n, seed=7)
    x0 = xs + np.random.default_rng(4).standard_normal((3, n))
    lo, hi = np.full((3, n), -np.inf), np.full((3, n), np.inf)
    held = np.zeros((3, n), dtype=bool)
    held[0, 4] = held[1, 0] = held[1, 2] = True
    lo[held] = hi[held] = x0[held] + 0.25                              # (not the start value: the start is projected onto it)
    mc = factory(x0, None, lo, hi, gtol=1e-6, maxiter=200)
    calls = 0
    while (mc.status == 0).any() and calls < 300:
        live = mc.status == 0
        fixed = held & live[:, None]
        assert np.array_equal(bits(mc.trial[fixed]), bits(lo[fixed])), "a variable with lo == hi moved"
        mc.advance(*fun(mc.trial))
        calls += 1
    assert (mc.status == 1).all(), mc.status
    assert np.array_equal(bits(mc.x[held]), bits(lo[held]))
    g = fun(mc.x)[1]
    assert np.abs(g[~held]).max() <= 1e-6 and np.abs(g[held]).min() > 1e-3


def check_one_sided(factory):
    """one-sided bounds (-inf / +inf on the other side): the separable answer max(c, lo) resp. min(c, hi), status 1"""
    rng = np.random.default_rng(77)
    C, n = 9, 6
    a = np.exp(rng.uniform(-1.0, 1.0, (C, n)))
    c = rng.uniform(-3.0, 3.0, (C, n))
    lo, hi = np.full((C, n), -np.inf), np.full((C, n), np.inf)
    lo[:, :3] = rng.uniform(-1.0, 1.0, (C, 3))                         # variables 0 .. 2: lower bound only
    hi[:, 3:5] = rng.uniform(-1.0, 1.0, (C, 2))                        # 3, 4: upper bound only; 5: free
    x0 = rng.uniform(-3.0, 3.0, (C, n))
    mc = factory(x0, None, lo, hi, gtol=1e-9, maxiter=200)
    calls = lc.drive(mc, separable(a, c), 400)
    assert (mc.status == 1).all(), (mc.status, calls)
    want = project(c, lo, hi)
    clipped = want != c
    assert clipped.sum() >= 10 and np.array_equal(bits(mc.x[clipped]), bits(want[clipped]))
    assert np.abs(mc.x - want).max() <= 1e-9 / np.exp(-1.0)


def check_bad_bounds(factory):
    """a row with lo_i > hi_i, and a row with a NaN bound, are done at once with status 5 and a NaN trial row, and stay so, while
    their neighbours converge"""
    fun, xs, A = lc.quadratic(5, seed=5)
    x0 = xs + np.random.default_rng(3).standard_normal((5, 5))
    lo, hi = np.full((5, 5), -4.0), np.full((5, 5), 4.0)
    lo[1, 2], hi[1, 2] = 1.0, 0.5
    hi[3, 0] = np.nan
    mc = factory(x0, None, lo, hi, gtol=1e-8)
    assert list(mc.status) == [0, 5, 0, 5, 0]
    assert np.isnan(mc.trial[[1, 3]]).all() and not np.isnan(mc.trial[[0, 2, 4]]).any()
    lc.drive(mc, fun, 200)
    assert list(mc.status) == [1, 5, 1, 5, 1] and (mc.evals[[1, 3]] == 0).all() and (mc.iters[[1, 3]] == 0).all()


ALL_CHECKS = ("separable", "coupled", "invariants", "start_rows", "lo_equals_hi", "one_sided", "bad_bounds")


def run_check(name, factory):
    return globals()["check_" + name](factory)


# ---- the inputs of the bit-identity tests (host program, device kernels) -------------------------------------------------------------
def identity_case(n, m, kind, C, ncalls=25, seed=0):
    """lbfgs_checks.identity_case with a box: the same rows (row 1 starts at NaN, row 2 is handed gradients of the wrong sign, row 4
    starts at the minimiser of its unbounded problem, every third row has its last variable masked) in per-row boxes around the
    start that cut the path off - rows hit bounds, reject, reset and finish -, every fifth variable with an infinite side, and (as
    far as C allows) row 3 with lo > hi in one variable and row 5 with a NaN bound.  A dict like lbfgs_checks.identity_case's, plus
    lo and hi."""
    base = lc.identity_case(n, m, kind, C, ncalls=1, seed=seed)       # (its x0, mask and rows)
    x0, mask, lam = base["x0"], base["mask"], base["lam"]
    rows = lc.sample_rows(n, 100 * n + seed)
    rng = np.random.default_rng(5000 + 1000 * n + 10 * m + kind + C)
    centre = np.where(np.isnan(x0), 0.0, x0)
    lo = centre - rng.uniform(-0.1, 0.4, (C, n))                      # some starts outside the box
    hi = np.maximum(centre + rng.uniform(-0.1, 0.4, (C, n)), lo + 0.05)
    flat = np.arange(C * n).reshape(C, n)
    lo[flat % 5 == 0] = -np.inf
    hi[flat % 5 == 3] = np.inf
    if C > 3:
        lo[3, n // 2], hi[3, n // 2] = 0.5, 0.25
    if C > 5:
        lo[5, 0] = np.nan

    def ab(x):
        mean, moment = rows(x)
        if kind == 0:
            a, b = np.concatenate([1.0 - mean[:, :1], -mean[:, 1:]], axis=1), np.zeros_like(mean)
        else:
            a, b = mean.copy(), (moment if kind == 2 else np.zeros_like(mean))
        if C > 2:
            a[2, 1:] = -a[2, 1:]
        return a, b
    mc = lbfgs.LBFGS(m=m, **lc.IDENTITY_PARAMS).init(x0, mask, lo, hi)
    case = {"n": n, "m": m, "kind": kind, "C": C, "lam": lam, "x0": x0, "mask": mask, "lo": lo, "hi": hi,
            "params": dict(lc.IDENTITY_PARAMS), "init": (mc.state_array(), mc.trial.copy()), "calls": []}
    counters = {"rejected": 0, "on_bound": 0, "reset": 0}
    for _ in range(ncalls):
        had = mc.count > 0
        it = mc.iters.copy()
        a, b = ab(mc.trial)
        with np.errstate(all="ignore"):
            mc.advance(*lbfgs.objective(kind, a, b, lam))
        case["calls"].append((a, b, mc.state_array(), mc.trial.copy()))
        counters["rejected"] += int(mc.rejected.sum())
        counters["reset"] += int((had & (mc.count == 0) & (mc.iters == it)).sum())
        live = mc.status == 0
        counters["on_bound"] += int(((mc.trial[live] == lo[live]) | (mc.trial[live] == hi[live])).sum())
    case["status"] = mc.status.copy()
    case["counters"] = counters
    return case
