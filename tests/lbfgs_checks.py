"""Checks of the batched L-BFGS state machine with analytic objectives evaluated on the host, written against any MACHINE: the
definition (`lbfgs.LBFGS`), the device kernels behind `backend.lbfgs_advance` (tests/test_gpu_lbfgs.py wraps them) and the broken
stand-ins of tests/test_lbfgs_checks.py, each of which one of the checks must catch.

A machine is made by `factory(x0, mask, **params)` and has `advance(ft, gt)` and, as NumPy arrays refreshed by every call,
`trial`, `x`, `f`, `g`, `status`, `iters`, `evals`, `nback`, `count`, `head` (the fields of `lbfgs.LBFGS`)."""
import importlib

import numpy as np

lbfgs = importlib.import_module("code-robchar_amd.lbfgs")

FIELDS = ("x", "f", "g", "d", "t", "gd", "S", "Y", "sy", "count", "head", "nback", "iters", "evals", "fprev", "status", "first", "mask")


def definition(x0, mask=None, **params):
    return lbfgs.LBFGS(**params).init(x0, mask)


# ---- objectives: x (C, n) -> (f (C,), g (C, n)); a NaN row gives NaN ----------------------------------------------------------
def quadratic(n, seed=0, cond=30.0):
    """f = 1/2 (x - x*)^T A (x - x*), A symmetric positive definite with eigenvalues in [1, cond]; returns (fun, x*, A)"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * np.geomspace(1.0, cond, n)) @ Q.T
    A = 0.5 * (A + A.T)
    xs = rng.standard_normal(n)

    def fun(x):
        r = x - xs
        Ar = r @ A
        return 0.5 * np.einsum("ci,ci->c", r, Ar), Ar
    return fun, xs, A


def rosenbrock(x):
    a, b = x[:, :-1], x[:, 1:]
    f = (100.0 * (b - a * a) ** 2 + (1.0 - a) ** 2).sum(axis=1)
    g = np.zeros_like(x)
    g[:, :-1] += -400.0 * a * (b - a * a) - 2.0 * (1.0 - a)
    g[:, 1:] += 200.0 * (b - a * a)
    return f, g


def drive(machine, fun, max_calls, stop=None):
    """call `advance` with the objective at `trial` until no row runs (or `max_calls`); returns the number of calls.  The rows of
    a done machine row are NaN in `trial`: the objective then returns NaN there, as the gradient kernels do."""
    calls = 0
    with np.errstate(all="ignore"):
        while (machine.status == 0).any() and calls < max_calls:
            ft, gt = fun(machine.trial)
            machine.advance(ft, gt)
            calls += 1
            if stop is not None and stop(machine):
                break
    return calls


# ---- an independent textbook L-BFGS of ONE row: a deque of pairs, np.dot - no ring, no masks over rows ---------------------------
def textbook_trials(fun, x0, ncalls, m=5, c1=1e-4, maxback=20):
    """the trial points the first `ncalls` calls leave behind, by the rules of the issue, for a row that never finishes in them"""
    from collections import deque
    step0 = lambda g: min(1.0, 1.0 / np.sqrt(g @ g))
    hist = deque(maxlen=m)
    one = lambda x: tuple(v[0] for v in fun(x[None, :]))
    trial = np.array(x0, dtype=np.float64)
    out = []
    x = f = g = d = t = None
    nback = 0
    for call in range(ncalls):
        ft, gt = one(trial)
        if call == 0:
            x, f, g = trial, ft, gt
            d, t = -g, step0(g)
        elif np.isfinite(ft) and ft <= f + c1 * t * (g @ d):
            s, y = trial - x, gt - g
            if s @ y > 0 and s @ y >= 1e-10 * np.sqrt(s @ s) * np.sqrt(y @ y):
                hist.append((s, y))
            x, f, g = trial, ft, gt
            q, al = g.copy(), []
            for s, y in reversed(hist):
                a = (s @ q) / (s @ y)
                al.append(a)
                q = q - a * y
            if hist:
                s, y = hist[-1]
                q = q * ((s @ y) / (y @ y))
            for (s, y), a in zip(hist, reversed(al)):
                q = q + (a - (y @ q) / (s @ y)) * s
            d, t, nback = -q, 1.0, 0
            if not hist or g @ d >= 0:
                hist.clear()
                d, t = -g, step0(g)
        else:
            nback += 1
            if nback > maxback:
                assert hist, "the textbook row fails its line search: choose another case"
                hist.clear()
                d, t, nback = -g, step0(g), 0
            else:
                t = t / 2
        trial = x + t * d
        out.append(trial)
    return np.array(out)


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
def check_quadratic(factory, n=6, C=5, m=5):
    """a convex quadratic with a known minimiser: every row ends with status 1 at the minimiser"""
    fun, xs, A = quadratic(n, seed=n)
    x0 = xs + 3.0 * np.random.default_rng(1).standard_normal((C, n))
    gtol = 1e-9
    mc = factory(x0, None, m=m, gtol=gtol, maxiter=200)
    calls = drive(mc, fun, 400)
    assert (mc.status == 1).all(), (mc.status, calls)
    # |g|_inf <= gtol and g = A (x - x*): |x - x*|_2 <= |A^-1|_2 sqrt(n) gtol = sqrt(n) gtol (smallest eigenvalue 1)
    assert np.abs(mc.x - xs).max() <= np.sqrt(n) * gtol
    assert (mc.evals == calls).any() and (mc.iters >= 1).all() and (mc.iters < mc.evals).all()
    assert np.isnan(mc.trial).all()
    return calls


ROSEN_X0 = np.array([[-1.2, 1.0, -1.2, 1.0], [2.0, -2.0, 2.0, -2.0], [0.0, 0.0, 0.0, 0.0], [-3.0, 4.0, 1.5, -0.5]])


ROSEN_LOCAL = np.array([-0.775659226408, 0.613093365215, 0.382062845998, 0.145972018307])    # the local minimum of n = 4


def check_rosenbrock(factory, m=5):
    """Rosenbrock in n = 4: every row reaches a minimum - the first three (1, 1, 1, 1), the last one that or the function's local
    minimum near (-0.78, 0.61, 0.38, 0.15); backtracking and a skipped pair occur on the way (the
    counters are asserted, so the case cannot go vacuous), and the accepted values never increase"""
    mc = factory(ROSEN_X0, None, m=m, gtol=1e-8, maxiter=500)
    rejected = skipped = 0
    prev_f = None
    calls = 0
    while (mc.status == 0).any() and calls < 1500:
        before = (mc.iters.copy(), mc.head.copy(), mc.count.copy(), mc.nback.copy(), mc.status.copy(), mc.sy.copy())
        prev_f = mc.f.copy()
        with np.errstate(all="ignore"):
            mc.advance(*rosenbrock(mc.trial))
        calls += 1
        acc = mc.iters > before[0]
        run = before[4] == 0
        rejected += int((run & ~acc & (before[0] > 0)).sum())
        # an accepted step whose pair was not stored: the ring is as it was
        same_ring = (mc.head == before[1]) & (mc.count == before[2]) & (mc.sy == before[5]).all(axis=1)
        skipped += int((acc & same_ring).sum())
        assert (mc.f[acc] <= prev_f[acc]).all(), "an accepted value above its predecessor"
    assert (mc.status == 1).all(), (mc.status, calls)
    err = np.minimum(np.abs(mc.x - 1.0).max(axis=1), np.abs(mc.x - ROSEN_LOCAL).max(axis=1))
    assert err.max() <= 1e-6 and np.abs(mc.x[:3] - 1.0).max() <= 1e-6, (err, mc.x)
    assert rejected > 0, "no backtracking step: the case is vacuous"
    assert skipped > 0, "no skipped pair: the case is vacuous"
    return rejected, skipped


def check_wrong_sign(factory, maxback=6):
    """a gradient with the wrong sign: status 4 within 2 (maxback + 1) + 2 calls; with the sign turning wrong only below a value,
    after pairs have been stored: one history reset (count back to 0), then status 4, within that many calls of the turn"""
    fun, xs, A = quadratic(4, seed=3)
    x0 = xs + np.random.default_rng(2).standard_normal((3, 4))
    wrong = lambda x: (fun(x)[0], -fun(x)[1])
    mc = factory(x0, None, m=3, maxback=maxback, gtol=1e-12)
    calls = drive(mc, wrong, 10 * maxback + 100)
    assert (mc.status == 4).all(), mc.status
    assert calls <= 2 * (maxback + 1) + 2, calls
    f0 = fun(x0)[0]

    def turning(x):
        f, g = fun(x)
        return f, np.where((f < 0.05 * f0.min())[:, None], -g, g)
    mc = factory(x0, None, m=3, maxback=maxback, gtol=1e-12)
    seen_pairs = np.zeros(3, dtype=bool)
    reset = np.zeros(3, dtype=bool)
    since = np.zeros(3, dtype=int)
    calls = 0
    while (mc.status == 0).any() and calls < 400:
        had = mc.count > 0
        it = mc.iters.copy()
        running = mc.status == 0
        with np.errstate(all="ignore"):
            mc.advance(*turning(mc.trial))
        calls += 1
        seen_pairs |= had
        reset |= had & (mc.count == 0) & (mc.iters == it)          # dropped by the line search, not by an accepted step
        since = np.where(mc.iters > it, 0, since + running)
        assert (since <= 2 * (maxback + 1) + 2).all(), since
    assert (mc.status == 4).all() and seen_pairs.all() and reset.all(), (mc.status, seen_pairs, reset)


def check_nan_start(factory):
    """a NaN start row is done at once with status 5 and a NaN trial row, and stays so, while its neighbours converge"""
    fun, xs, A = quadratic(5, seed=5)
    x0 = xs + np.random.default_rng(3).standard_normal((4, 5))
    x0[2, 1] = np.nan
    mc = factory(x0, None, gtol=1e-8)
    assert mc.status[2] == 5 and np.isnan(mc.trial[2]).all() and not np.isnan(mc.trial[[0, 1, 3]]).any()
    drive(mc, fun, 200)
    assert list(mc.status) == [1, 1, 5, 1] and mc.evals[2] == 0 and mc.iters[2] == 0


def check_mask(factory):
    """a masked variable is bitwise unchanged in every trial point and in the result; the free ones reach the constrained minimum"""
    n = 5
    fun, xs, A = quadratic(n, seed=7)
    x0 = xs + np.random.default_rng(4).standard_normal((3, n))
    mask = np.ones((3, n))
    mask[0, n - 1] = mask[1, 0] = mask[1, 2] = 0.0
    # (gtol: the values stay of order 1 with a variable held, so a decrease of |g|^2 is resolved down to |g| ~ 1e-8 only)
    mc = factory(x0, mask, gtol=1e-6, maxiter=200)
    calls = 0
    while (mc.status == 0).any() and calls < 300:
        live = mc.status == 0
        fixed = (mask == 0.0) & live[:, None]
        assert np.array_equal(mc.trial[fixed].view(np.uint64), x0[fixed].view(np.uint64)), "a masked variable moved"
        mc.advance(*fun(mc.trial))
        calls += 1
    assert (mc.status == 1).all()
    assert np.array_equal(mc.x[mask == 0.0].view(np.uint64), x0[mask == 0.0].view(np.uint64))
    g = fun(mc.x)[1]
    assert np.abs(g[mask == 1.0]).max() <= 1e-6 and np.abs(g[mask == 0.0]).min() > 1e-3


def check_ring_wraps(factory, n=8, m=2, ncalls=14):
    """more than m accepted steps: the trial points follow an independent textbook L-BFGS (a deque of the last m pairs) to rounding"""
    fun, xs, A = quadratic(n, seed=11, cond=10.0)
    x0 = xs + np.random.default_rng(5).standard_normal((3, n))
    mc = factory(x0, None, m=m, gtol=1e-14)
    got = []
    for _ in range(ncalls):
        mc.advance(*fun(mc.trial))
        got.append(mc.trial.copy())
    got = np.array(got)
    assert (mc.iters > m + 2).all() and (mc.status == 0).all(), (mc.iters, mc.status)
    for c in range(3):
        want = textbook_trials(fun, x0[c], ncalls, m=m)
        # the two differ in summation order only: ~n eps per dot product, amplified by at most the condition number (10) per
        # step over 14 steps of a contracting iteration; 1e-9 of the scale of x leaves six digits of room
        assert np.abs(got[:, c] - want).max() <= 1e-9 * np.abs(want).max(), (c, np.abs(got[:, c] - want).max())


def check_frozen(factory, snapshot):
    """rows that finish at different calls: from the call that ends a row on, its state (`snapshot(machine)`: every field of the
    row) is frozen and its trial row is NaN while its neighbours go on"""
    n = 4
    fun, xs, A = quadratic(n, seed=13)
    rng = np.random.default_rng(6)
    x0 = xs + rng.standard_normal((6, n)) * np.array([1e-7, 1e-3, 1.0, 10.0, 1e-5, 100.0])[:, None]
    mc = factory(x0, None, gtol=1e-6, maxiter=200)
    done_at = np.full(6, -1)
    frozen = {}
    calls = 0
    while (mc.status == 0).any() and calls < 300:
        mc.advance(*fun(mc.trial))
        calls += 1
        snap = snapshot(mc)
        for c in np.nonzero(mc.status != 0)[0]:
            if done_at[c] < 0:
                done_at[c] = calls
                frozen[c] = snap[:, c].copy()
            assert np.array_equal(snap[:, c], frozen[c], equal_nan=True), f"row {c} changed after it was done"
            assert np.isnan(mc.trial[c]).all(), f"row {c}: done, but its trial row is not NaN"
        assert not np.isnan(mc.trial[mc.status == 0]).any()
    assert (mc.status == 1).all() and len(set(done_at)) >= 3, done_at


ALL_CHECKS = ("quadratic", "rosenbrock", "wrong_sign", "nan_start", "mask", "ring_wraps", "frozen")


def run_check(name, factory, snapshot=lambda mc: mc.state_array()):
    if name == "frozen":
        return check_frozen(factory, snapshot)
    return globals()["check_" + name](factory)


# ---- the known answer: perfect state transfer 0 -> 2 of the uniform 3-chain ---------------------------------------------------------
def chain3_one_minus_fidelity(x, inspin=0, outspin=2):
    """1 - F and its gradient for controller rows x = (B_0, B_1, B_2, T) of the 3-chain with unit couplings, F = |<out| exp(-i H T)
    |in>|^2, H = tridiag(1; B): NumPy eigendecomposition, dF/dB_k by the divided differences of exp(-i lambda T) (Daleckii - Krein)"""
    x = np.asarray(x, dtype=np.float64)
    C, N = x.shape[0], x.shape[1] - 1
    f = np.full(C, np.nan)
    g = np.full((C, N + 1), np.nan)
    for c in range(C):
        if not np.isfinite(x[c]).all():
            continue
        B, T = x[c, :N], x[c, N]
        H = np.diag(B) + np.diag(np.ones(N - 1), 1) + np.diag(np.ones(N - 1), -1)
        lam, V = np.linalg.eigh(H)
        e = np.exp(-1j * lam * T)
        amp = (V[outspin] * e) @ V[inspin]
        dl = lam[:, None] - lam[None, :]
        close = np.abs(dl) < 1e-9
        dd = np.where(close, -1j * T * e[:, None], (e[:, None] - e[None, :]) / np.where(close, 1.0, dl))
        for k in range(N):
            M = np.outer(V[k], V[k])                                  # V^T dH/dB_k V
            damp = (V[outspin][:, None] * dd * M * V[inspin][None, :]).sum()
            g[c, k] = -2.0 * (np.conj(amp) * damp).real
        damp_T = (V[outspin] * (-1j * lam * e)) @ V[inspin]
        g[c, N] = -2.0 * (np.conj(amp) * damp_T).real
        f[c] = 1.0 - abs(amp) ** 2
    return f, g


def known_answer_start(C=16, seed=0):
    x0 = np.empty((C, 4))
    x0[:, :3] = 0.05 * np.random.default_rng(seed).standard_normal((C, 3))
    x0[:, 3] = np.pi / np.sqrt(2.0) + 0.1
    return x0


def check_known_answer(factory):
    """N = 3, 0 -> 2, no noise, from biases 0.05 N(0, 1) and T = pi / sqrt(2) + 0.1: every row reaches 1 - F <= 1e-10 with status 1
    within 12 evaluations at gtol = 1e-7"""
    mc = factory(known_answer_start(), None, gtol=1e-7)
    calls = drive(mc, chain3_one_minus_fidelity, 12)
    print("known answer: evals", mc.evals, "max 1 - F", mc.f.max())
    assert (mc.status == 1).all(), (mc.status, calls)
    assert (mc.evals <= 12).all() and (mc.f <= 1e-10).all(), (mc.evals, mc.f)


# ---- the inputs of the bit-identity tests (host program, device kernels): rows a gradient entry would write ------------------------
IDENTITY_PARAMS = {"c1": 1e-4, "gtol": 1e-5, "ftol": 1e-7, "maxiter": 12, "maxback": 5}
IDENTITY_LAM = 1.0


def sample_rows(n, seed):
    """x (C, n) -> (mean (C, n + 1), moment (C, n + 1)) of three smooth "fidelities" F_k = 1 / (1 + q_k(x)), q_k convex quadratics
    with different minimisers: the "mean" and "moment" rows of the gradient entries, NaN for a NaN row"""
    quads = [quadratic(n, seed=seed + k, cond=5.0)[0] for k in range(3)]

    def rows(x):
        with np.errstate(all="ignore"):
            F, dF = [], []
            for q in quads:
                v, gq = q(x)
                F.append(1.0 / (1.0 + v))
                dF.append(-gq / ((1.0 + v) ** 2)[:, None])
            F, dF = np.array(F), np.array(dF)
            mean = np.concatenate([F.mean(axis=0)[:, None], dF.mean(axis=0)], axis=1)
            moment = np.concatenate([(F * F).mean(axis=0)[:, None], (F[:, :, None] * dF).mean(axis=0)], axis=1)
        return mean, moment
    return rows


def identity_case(n, m, kind, C, ncalls=25, seed=0):
    """One case of the bit-identity tests: a dict with x0, mask, the parameters and, per call, the rows (a, b) handed to `advance`
    and the definition's state and trial after it.  Among the rows (as far as C allows): row 1 starts at NaN, row 2 is handed
    gradients of the wrong sign, row 4 starts at the minimiser (done at its first call), every third row has its last variable
    masked; the others end by gtol, ftol or maxiter at different calls or are still running."""
    rows = sample_rows(n, 100 * n + seed)
    rng = np.random.default_rng(1000 * n + 10 * m + kind + C)
    x0 = 0.7 * rng.standard_normal((C, n))
    mask = np.ones((C, n))
    mask[::3, n - 1] = 0.0
    lam = IDENTITY_LAM if kind == 2 else 0.0

    def ab(x, flip):
        mean, moment = rows(x)
        if kind == 0:
            a, b = np.concatenate([1.0 - mean[:, :1], -mean[:, 1:]], axis=1), np.zeros_like(mean)
        else:
            a, b = mean.copy(), (moment if kind == 2 else np.zeros_like(mean))
        if flip and C > 2:                                    # (kind 2: the wrong sign in the mean's gradient alone)
            a[2, 1:] = -a[2, 1:]
        return a, b
    if C > 4:                                                 # the minimiser of row 4's own problem (unmasked: 4 % 3 != 0)
        one = lbfgs.LBFGS(m=5, gtol=1e-12, maxiter=500).init(x0[4:5], None)
        for _ in range(400):
            if not one.running():
                break
            a, b = (v[:1] for v in ab(np.repeat(one.trial, C, axis=0), False))
            one.advance(*lbfgs.objective(kind, a, b, lam))
        x0[4] = one.x[0]
    if C > 1:
        x0[1, n // 2] = np.nan
    mc = lbfgs.LBFGS(m=m, **IDENTITY_PARAMS).init(x0, mask)
    case = {"n": n, "m": m, "kind": kind, "C": C, "lam": lam, "x0": x0, "mask": mask, "params": dict(IDENTITY_PARAMS),
            "init": (mc.state_array(), mc.trial.copy()), "calls": []}
    for _ in range(ncalls):
        a, b = ab(mc.trial, True)
        mc.advance(*lbfgs.objective(kind, a, b, lam))
        case["calls"].append((a, b, mc.state_array(), mc.trial.copy()))
    case["status"] = mc.status.copy()
    return case
