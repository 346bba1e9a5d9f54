"""Batched L-BFGS with a backtracking (Armijo) line search, one independent problem per row: the DEFINITION of the device state
machine behind `rc_lbfgs_init_f64_async` / `rc_lbfgs_advance_f64_async` (csrc/lbfgs_core.h, csrc/k_lbfgs.inc.h), in plain NumPy
over all rows at once.  The kernel gives these bits.

A row has n variables and minimises a value f with gradient g.  The caller evaluates (f, g) at the rows of `trial` - for the
product that is one gradient launch over all controller rows - and hands them to `advance`, which decides per row: first value,
accept, or backtrack, and writes the next `trial`.  Rows are in different phases in the same call.  A row whose `status` is not 0
is DONE: its `trial` row is all NaN (the gradient kernels skip a NaN controller row), its state never changes again, and `x`, `f`,
`g` are its result.

    status   0 running                     1 max |g_i| <= gtol           2 fprev - f <= ftol max(|fprev|, |f|, 1)   (ftol = 0: off)
             3 iters = maxiter             4 line search failed          5 first value or gradient not finite, or a NaN start row
                                                                           (boxed: or bad bounds)

Bit-identity rules.  Every dot product and norm is accumulated SEQUENTIALLY over the variable index from 0.0
(`acc = acc + a[:, i] * b[:, i]`), every product is rounded once before it is added (no fused multiply-add), divisions and
square roots are the IEEE operations.  A NaN is a NaN: its sign and payload are not part of the definition.

Constraints.  The 0 / 1 `mask`: a masked variable never moves (fix the time T this way).  Box bounds: `init(x0, mask, lo, hi)` with
`lo`, `hi` broadcastable to (C, n), -inf / +inf allowed per entry, selects the BOXED variant of the machine; without them everything
is the unbounded machine, bit for bit.  With P(v) = where(v < lo, lo, where(v > hi, hi, v)) (a NaN stays a NaN) the boxed rules are

    start     x0 <- P(x0), masked variables included; a row with a NaN bound or lo_i > hi_i is done at once with status 5
    accept    s = trial - x, gs = g.s: accept iff ft is finite and gs < 0 and ft <= f + c1 gs (gs < 0 keeps a clipped quasi-Newton
              step from being accepted uphill; as t -> 0 the step is t d on the free variables and gs -> t gd < 0)
    pair      s is the projected step, y = gt - g; the store rule is unchanged
    status 1  max_i |x_i - P(x - g)_i| <= gtol (the projected gradient of L-BFGS-B); statuses 2 to 5 are unchanged
    direction at every new direction the active set A_i = (x_i <= lo_i and g_i > 0) or (x_i >= hi_i and g_i < 0) is recomputed;
              gr = g with the A entries 0; the two-loop recursion starts from q = gr; dq = -q with the A entries 0, gdq = g.dq; the
              quasi-Newton direction is taken iff count > 0 and not gdq >= 0, otherwise steepest descent -gr with first_step(gr)
              and the history dropped; gd = g.d
    trial     P(x + t d), on a new direction and after every halving; reject, maxback, the one-time reset and status 4 are unchanged

Nothing new is stored: `lo` and `hi` are inputs of `init` and of every `advance` (the device entries take the same two arrays each
time; this class keeps them from `init`).  L-BFGS-B's Cauchy point and subspace minimisation are out of scope.

The state as the device keeps it is `state_array()`: (state_fields(n, m), C) doubles, field-major, the fields in the order of
`field_offsets`; integers are stored as doubles."""
from __future__ import annotations

import numpy as np

KINDS = {"raw": 0, "one_minus": 1, "one_minus_plus_std": 2}
MIN_DIM, MAX_DIM, MAX_M = 3, 13, 8
PAIR_EPS = 1e-10                      # a pair is stored when sy > 0 and sy >= PAIR_EPS sqrt(ss) sqrt(yy)
VAR_FLOOR = 64.0 * 2.0 ** -52         # `noise.moments_from_sums`
DEFAULTS = {"m": 5, "c1": 1e-4, "gtol": 1e-6, "ftol": 0.0, "maxiter": 100, "maxback": 20}


def field_offsets(n: int, m: int) -> dict:
    """Name -> first row of the field in the (fields, C) state; "len" = number of rows (csrc/lbfgs_core.h: rclb::Layout)."""
    off, o = {}, 0
    for name, size in (("x", n), ("f", 1), ("g", n), ("d", n), ("t", 1), ("gd", 1), ("S", m * n), ("Y", m * n), ("sy", m),
                       ("count", 1), ("head", 1), ("nback", 1), ("iters", 1), ("evals", 1), ("fprev", 1), ("status", 1),
                       ("first", 1), ("mask", n)):
        off[name] = o
        o += size
    off["len"] = o
    return off


def state_fields(n: int, m: int) -> int:
    return 4 * n + 2 * m * n + m + 11


def _dot(a, b):
    acc = np.zeros(a.shape[0])
    for i in range(a.shape[1]):
        acc = acc + a[:, i] * b[:, i]
    return acc


def _absmax(g):
    acc = np.zeros(g.shape[0])
    for i in range(g.shape[1]):
        v = np.abs(g[:, i])
        acc = np.where(v > acc, v, acc)                  # (a NaN is never taken)
    return acc


def first_step(g):
    """min(1, 1 / ||g||_2) per row: the first trial step along -g."""
    with np.errstate(all="ignore"):
        r = 1.0 / np.sqrt(_dot(g, g))
        return np.where(r < 1.0, r, 1.0)


def objective(kind, a, b=None, lam: float = 0.0):
    """(ft (C,), gt (C, n)) from the rows the gradient entries write, n = a.shape[1] - 1.

    "raw"                 a = (f, g_0 .. g_{n-1}) as they are
    "one_minus"           a = a `mean` row of mc_fidelity_grad[_philox] or a `sum` row of mc_fidelity_grad_listed: f = 1 - a[0], g = -a[1:]
    "one_minus_plus_std"  a = mean, b = moment: f = (1 - fav) + lam std, g = -grad_fav + lam grad_std, std and grad_std by the
                          arithmetic of `noise.moments_from_sums` with its floor rule."""
    kind = KINDS[kind] if isinstance(kind, str) else int(kind)
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(all="ignore"):
        if kind == 0:
            return a[:, 0].copy(), a[:, 1:].copy()
        if kind == 1:
            return 1.0 - a[:, 0], -a[:, 1:]
        if kind != 2:
            raise ValueError("kind: raw, one_minus or one_minus_plus_std")
        b = np.asarray(b, dtype=np.float64)
        lam = float(lam)
        fav, m2 = a[:, 0], b[:, 0]
        var = m2 - fav * fav
        floor = var <= VAR_FLOOR * m2
        var = np.where(floor, 0.0, var)
        std = np.sqrt(var)
        safe = np.where(floor, 1.0, std)
        g = np.empty_like(a[:, 1:])
        for i in range(g.shape[1]):
            grad_var = 2.0 * (b[:, 1 + i] - fav * a[:, 1 + i])
            grad_std = np.where(floor, 0.0, grad_var / (2.0 * safe))
            g[:, i] = -a[:, 1 + i] + lam * grad_std
        return (1.0 - fav) + lam * std, g


class LBFGS:
    """The state of C rows.  `init(x0, mask)` - or `init(x0, mask, lo, hi)` for the boxed variant - then `advance(ft, gt)` with
    (ft, gt) evaluated at `self.trial`, until `running()` is False; the result is `x`, `f`, `g`, `status`, `iters`, `evals`."""

    def __init__(self, m: int = 5, c1: float = 1e-4, gtol: float = 1e-6, ftol: float = 0.0, maxiter: int = 100, maxback: int = 20):
        if not 1 <= int(m) <= MAX_M:
            raise ValueError(f"m must be 1 .. {MAX_M}")
        self.m, self.c1, self.gtol, self.ftol = int(m), float(c1), float(gtol), float(ftol)
        self.maxiter, self.maxback = int(maxiter), int(maxback)

    def _project(self, v):
        return np.where(v < self.lo, self.lo, np.where(v > self.hi, self.hi, v))

    def _stationarity(self):
        """what status 1 compares with gtol: max |g_i|, boxed max |x_i - P(x - g)_i|"""
        return _absmax(self.x - self._project(self.x - self.g)) if self.box else _absmax(self.g)

    def init(self, x0, mask=None, lo=None, hi=None):
        x0 = np.array(x0, dtype=np.float64)
        if x0.ndim != 2 or not MIN_DIM <= x0.shape[1] <= MAX_DIM:
            raise ValueError(f"x0: expected (C, n), n = {MIN_DIM} .. {MAX_DIM}")
        C, n = x0.shape
        self.C, self.n = C, n
        self.mask = np.ones((C, n)) if mask is None else np.array(np.broadcast_to(np.asarray(mask, dtype=np.float64), (C, n)))
        bad = np.isnan(x0).any(axis=1)
        self.box = lo is not None or hi is not None
        self.lo = self.hi = None
        if self.box:
            self.lo = np.array(np.broadcast_to(np.asarray(-np.inf if lo is None else lo, dtype=np.float64), (C, n)))
            self.hi = np.array(np.broadcast_to(np.asarray(np.inf if hi is None else hi, dtype=np.float64), (C, n)))
            bad = bad | np.isnan(self.lo).any(axis=1) | np.isnan(self.hi).any(axis=1) | (self.lo > self.hi).any(axis=1)
            x0 = self._project(x0)
        self.x = x0.copy()
        self.f = np.full(C, np.nan)
        self.g = np.full((C, n), np.nan)
        self.d = np.zeros((C, n))
        self.t = np.zeros(C)
        self.gd = np.zeros(C)
        self.S = np.zeros((C, self.m, n))
        self.Y = np.zeros((C, self.m, n))
        self.sy = np.zeros((C, self.m))
        self.count = np.zeros(C, dtype=np.int64)
        self.head = np.zeros(C, dtype=np.int64)
        self.nback = np.zeros(C, dtype=np.int64)
        self.iters = np.zeros(C, dtype=np.int64)
        self.evals = np.zeros(C, dtype=np.int64)
        self.fprev = np.full(C, np.nan)
        self.status = np.where(bad, 5, 0).astype(np.int64)
        self.first = np.ones(C, dtype=np.int64)
        self.trial = np.where(bad[:, None], np.nan, x0)
        return self

    def running(self) -> bool:
        return bool((self.status == 0).any())

    def state_array(self):
        """The (fields, C) array of the device state buffer."""
        C = self.C
        rows = [self.x.T, self.f[None], self.g.T, self.d.T, self.t[None], self.gd[None],
                self.S.reshape(C, -1).T, self.Y.reshape(C, -1).T, self.sy.T]
        rows += [v[None].astype(np.float64) for v in (self.count, self.head, self.nback, self.iters, self.evals)]
        rows += [self.fprev[None], self.status[None].astype(np.float64), self.first[None].astype(np.float64), self.mask.T]
        return np.ascontiguousarray(np.concatenate(rows, axis=0))

    def advance(self, ft, gt):
        m, C = self.m, self.C
        ar = np.arange(C)
        with np.errstate(all="ignore"):
            ft = np.array(ft, dtype=np.float64).reshape(C)
            gt = np.array(gt, dtype=np.float64).reshape(C, self.n) * self.mask
            run = self.status == 0
            self.evals = self.evals + run
            first = run & (self.first == 1)
            later = run & ~first
            self.first = np.where(first, 0, self.first)
            finite = np.isfinite(ft) & np.isfinite(gt).all(axis=1)
            start = first & finite
            self.status = np.where(first & ~finite, 5, self.status)
            s = self.trial - self.x
            if self.box:
                gs = _dot(self.g, s)
                accept = later & np.isfinite(ft) & (gs < 0.0) & (ft <= self.f + self.c1 * gs)
            else:
                accept = later & np.isfinite(ft) & (ft <= self.f + (self.c1 * self.t) * self.gd)
            reject = later & ~accept

            # accept: the pair (s, y)
            y = gt - self.g
            ss, yy, sy = _dot(s, s), _dot(y, y), _dot(s, y)
            store = accept & (sy > 0.0) & (sy >= (PAIR_EPS * np.sqrt(ss)) * np.sqrt(yy))
            rows = np.nonzero(store)[0]
            h = self.head[rows]
            self.S[rows, h], self.Y[rows, h], self.sy[rows, h] = s[rows], y[rows], sy[rows]
            self.head[rows] = (h + 1) % m
            self.count[rows] = np.minimum(self.count[rows] + 1, m)
            self.skipped = accept & ~store                 # (not state: for the tests' counters)
            moved = start | accept
            self.fprev = np.where(accept, self.f, self.fprev)
            self.x = np.where(moved[:, None], self.trial, self.x)
            self.f = np.where(moved, ft, self.f)
            self.g = np.where(moved[:, None], gt, self.g)
            self.iters = self.iters + accept
            st1 = moved & (self._stationarity() <= self.gtol)
            big = np.abs(self.fprev)
            big = np.where(np.abs(self.f) > big, np.abs(self.f), big)
            big = np.where(1.0 > big, 1.0, big)
            st2 = accept & ~st1 & (self.ftol > 0.0) & (self.fprev - self.f <= self.ftol * big)
            st3 = accept & ~st1 & ~st2 & (self.iters >= self.maxiter)
            self.status = np.where(st1, 1, np.where(st2, 2, np.where(st3, 3, self.status)))
            newdir = moved & (self.status == 0)

            # two-loop recursion over the stored pairs: newest first, then oldest first
            if self.box:                                   # the active set of the new direction (also of a reset's)
                active = ((self.x <= self.lo) & (self.g > 0.0)) | ((self.x >= self.hi) & (self.g < 0.0))
                gr = np.where(active, 0.0, self.g)
            else:
                gr = self.g
            q = gr.copy()
            alpha = np.zeros((C, m))
            for j in range(m):
                act = newdir & (j < self.count)
                slot = (self.head - 1 - j) % m
                a = (1.0 / self.sy[ar, slot]) * _dot(self.S[ar, slot], q)
                q = np.where(act[:, None], q - a[:, None] * self.Y[ar, slot], q)
                alpha[:, j] = a
            newest = (self.head - 1) % m
            h0 = self.sy[ar, newest] / _dot(self.Y[ar, newest], self.Y[ar, newest])
            q = np.where((newdir & (self.count > 0))[:, None], h0[:, None] * q, q)
            for j in range(m - 1, -1, -1):
                act = newdir & (j < self.count)
                slot = (self.head - 1 - j) % m
                b = (1.0 / self.sy[ar, slot]) * _dot(self.Y[ar, slot], q)
                q = np.where(act[:, None], q + (alpha[:, j] - b)[:, None] * self.S[ar, slot], q)
            dq = -q
            if self.box:
                dq = np.where(active, 0.0, dq)
            gdq = _dot(self.g, dq)

            # reject: halve, or after maxback halvings drop the history once, then give up
            self.nback = np.where(reject, self.nback + 1, self.nback)
            over = reject & (self.nback > self.maxback)
            reset = over & (self.count > 0)
            self.status = np.where(over & (self.count == 0), 4, self.status)
            self.t = np.where(reject & ~over, self.t * 0.5, self.t)

            quasi = newdir & (self.count > 0) & ~(gdq >= 0.0)
            steep = (newdir & ~quasi) | reset
            self.count = np.where(steep, 0, self.count)
            self.head = np.where(steep, 0, self.head)
            ds = -gr
            self.d = np.where(quasi[:, None], dq, np.where(steep[:, None], ds, self.d))
            self.gd = np.where(quasi, gdq, np.where(steep, _dot(self.g, ds), self.gd))
            self.t = np.where(quasi, 1.0, np.where(steep, first_step(gr), self.t))
            self.nback = np.where(newdir | reset, 0, self.nback)
            going = run & (self.status == 0)
            step = self.x + self.t[:, None] * self.d
            self.trial = np.where(going[:, None], self._project(step) if self.box else step, np.nan)
        self.accepted, self.rejected = accept, reject      # (not state: for the tests' counters)
        return self

    def result(self):
        return {"x": self.x.copy(), "f": self.f.copy(), "grad": self.g.copy(), "status": self.status.astype(np.int32),
                "iters": self.iters.copy(), "evals": self.evals.copy()}
